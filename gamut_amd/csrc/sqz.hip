// sqz.hip -- the SQZ back end on the GPU and the two batch calls: coefficient planes in HBM -> l8 / rgb8 pixels, bit for bit what
// SQZ_dwt_convert_from_sign_magnitude, SQZ_idwt and SQZ_color_process (source/gamut/codecs/sqz.d:1584-1592, 1699-1796, 1153-1546)
// make of them.  The front end (the bit stream) is sqz_host.hip on host threads or sqz_read.hip on the device, by gamut_hip_sqz_set_reader.
//
// THE REFERENCE'S ORDER, AND WHY A LEVEL IS DATA-PARALLEL.  SQZ_idwt_5_3i (:1743-1770) walks a level's rows in pairs: the vertical
// lifting of an even row r (r -= (n + s + 2) >> 2, n and s the odd rows around it), then of the odd row n above it (n += (nn + r) >> 1,
// both even neighbours already updated), then the horizontal pass of nn and of n.  A row's horizontal pass comes only after the last
// vertical step that reads the row (nn is read by n's step, n by r's step, both earlier in the same iteration), and the horizontal
// pass of a row reads that row alone.  So the level equals: all even rows' vertical step from the ORIGINAL odd rows, then all odd rows'
// step from the UPDATED even rows, then every row's horizontal pass.  SQZ_mirror and the pointer guards (n <= s, nn <= r) come to the
// usual symmetric extension: row -1 is row 1, row h is row h - 2 (traced for even and odd h; every level's sides are >= 8).  Each
// output depends on at most 3 rows x 3 columns of a level's input.
//
// THE HORIZONTAL PASS (:1699-1741) holds a row as [low half | high half] and writes it interleaved.  With ints e(i) = L[i] -
// ((H[i-1] + H[i] + 2) >> 2) (e(0) and, for an odd width, the last one use one neighbour: (H + 1) >> 1): even outputs are (short)e(i);
// odd outputs H[i] - (-(e(i) + e(i+1)) >> 1) use the UNTRUNCATED ints inside the reference's loop (i <= w - 2, w = width / 2 - 1) and
// the values read back from the short scratch row in its tail (i = w - 1, w).  The difference shows only when a coefficient leaves 16
// bits; it is kept.
//
// LAUNCHES.  One per level, deepest first, each over every image and plane of the batch that has that level (a table of unit counts
// per image, binary search per workgroup): at most eight, whatever the number of files.  A workgroup makes a 128 x 16 tile of the
// level's output from an LDS tile with its halo: 19 rows x (65 low + 66 high) columns.  Tiling rules out working in place (a tile's
// outputs are other tiles' inputs, and the horizontal pass permutes a row), so a level reads its detail bands from the caller's
// coefficient buffer (sign-magnitude, converted in the load: the fusion the first level wants holds for every level) and its LL
// quarter from where the level below wrote it, compact, in one of two scratch buffers used alternately.  Level 0 is not stored: its
// workgroup does the tile for all planes, keeps them in LDS and writes pixels (see DESIGN.md for why the colour stage is fused).
// The caller's coefficient buffer is only read today; the header keeps it "unspecified after the call".
#include "common.hpp"

namespace gamut {
bool sqz_valid_geometry(int64_t w, int64_t h, int mode, int scan, int levels);                   // sqz_host.hip
int  sqz_parse_header(const uint8_t* data, size_t len, gamut_hip_sqz_info* info);
int  sqz_decode_coeffs(const uint8_t* data, size_t len, int16_t* out, size_t capacity, gamut_hip_sqz_info* info);
const uint8_t* sqz_linear_to_srgb_table();
int  sqz_reader();                                                  // sqz_read.hip: 0 the host front end, 1 the device reader
int  sqz_read_files(const uint8_t* const* data, const size_t* len, const gamut_hip_sqz_info* info, const std::vector<int>& which,
                    int16_t* coeffs, const int64_t* coeff_offset, hipStream_t stream);
namespace {

constexpr int kThreads = 256, kTW = 128, kTH = 16, kRows = kTH + 3, kNL = kTW / 2 + 1, kNH = kTW / 2 + 2;

struct SqzImg {
    int64_t out_off, coeff_off, scratch_off;                        // bytes; int16 elements; int16 elements inside either scratch buffer
    uint32_t w, h, slot;                                            // slot: elements of one plane in a scratch buffer = ceil(w / 2) * ceil(h / 2)
    uint8_t levels, mode, planes, pad;
};

__device__ __forceinline__ int sm_to_int(int16_t v) { return (v & 1) ? -(v >> 1) : (v >> 1); }      // :1590 (|v >> 1| <= 16384: no wrap)
__device__ __forceinline__ int mirror(int v, int maximum)           // SQZ_mirror :513-526, maximum >= 7
{
    while ((uint32_t)v > (uint32_t)maximum) { v = -v; if (v < 0) v += 2 * maximum; }
    return v;
}
__device__ __forceinline__ uint32_t clip8(int16_t v) { return v < 0 ? 0u : v > 255 ? 255u : (uint32_t)v; }      // SQZ_COLOR_CLIP :1144-1151
__device__ __forceinline__ uint32_t linear_to_srgb(int32_t v, const uint8_t* t)                    // SQZ_linear_i32_to_sRGB_u8 :1323-1338
{
    if (v <= 0) return 0u;
    if (v >= 65535) return 255u;
    const int vmul = v * 511, off = vmul >> 16, frac = vmul & 65535, base = t[off];
    return (uint32_t)(base + ((frac * ((int)t[off + 1] - base)) >> 16)) & 0xFFu;
}
__device__ __forceinline__ int32_t wrap32(int64_t v) { return (int32_t)(uint32_t)(uint64_t)v; }     // cast(int) of a long

// one pixel: the three planes' values -> r | g << 8 | b << 16 (grey: the value alone)
__device__ __forceinline__ uint32_t colour(int mode, int16_t c0, int16_t c1, int16_t c2, const uint8_t* table)
{
    if (mode == 0) return clip8((int16_t)(c0 + 128));                                               // :1179-1180
    if (mode == 1) {                                                                                // YCoCg-R :1222-1230
        const int16_t Y = (int16_t)(c0 + 128);
        const int16_t B = (int16_t)(Y + ((1 - c2) >> 1) - (c1 >> 1));
        const int16_t G = (int16_t)(Y - ((-(int)c2) >> 1));
        const int16_t R = (int16_t)(c1 + B);
        return clip8(R) | clip8(G) << 8 | clip8(B) << 16;
    }
    if (mode == 2) {                                                                                // Oklab :1427-1439, 64-bit intermediates
        const int64_t L = (int16_t)(c0 + 2048), a = c1, b = c2;
        const int64_t l_ = L * 16 + ((25974LL * a + 14143LL * b) >> 12);
        const int64_t m_ = L * 16 + ((-6918LL * a - 4185LL * b) >> 12);
        const int64_t s_ = L * 16 + ((-5864LL * a - 84638LL * b) >> 12);
        const int64_t l = (l_ * l_ * l_) >> 32, m = (m_ * m_ * m_) >> 32, s = (s_ * s_ * s_) >> 32;
        return linear_to_srgb(wrap32((267169LL * l - 216771LL * m + 15137LL * s) >> 16), table)
             | linear_to_srgb(wrap32((-83127LL * l + 171030LL * m - 22368LL * s) >> 16), table) << 8
             | linear_to_srgb(wrap32((-275LL * l - 46099LL * m + 111909LL * s) >> 16), table) << 16;
    }
    const int Y = (int16_t)(c0 + 221);                                                              // LOG-L1 :1503-1511
    const int16_t R = (int16_t)((33779 * Y - 52830 * c1 + 19051 * c2) >> 16);
    const int16_t G = (int16_t)((41184 * Y + 8188 * c1 - 50317 * c2) >> 16);
    const int16_t B = (int16_t)((38182 * Y + 37906 * c1 + 37420 * c2) >> 16);
    return clip8(R) | clip8(G) << 8 | clip8(B) << 16;
}

// Level `level` of the batch.  first[i] .. first[i + 1]: the units (workgroups) of image i; FINAL (level 0): one unit per tile, all planes
// and the colour stage; otherwise one unit per plane and tile, written to scratch[level & 1].
template <bool FINAL>
__global__ __launch_bounds__(kThreads) void k_sqz_level(const SqzImg* __restrict__ imgs, const uint32_t* __restrict__ first, int count, int level,
                                                        const int16_t* __restrict__ coeffs, int16_t* __restrict__ scratch0, int16_t* __restrict__ scratch1,
                                                        const uint8_t* __restrict__ table_g, uint8_t* __restrict__ out)
{
    __shared__ int16_t lo[kRows][kNL + 1];
    __shared__ int16_t hi[kRows][kNH];
    __shared__ int16_t pix[FINAL ? 3 : 1][FINAL ? kTH : 1][FINAL ? kTW : 2];
    __shared__ uint8_t table[FINAL ? 512 : 4];
    const uint32_t tid = threadIdx.x, unit = blockIdx.x;
    int a = 0, b = count - 1;                                       // the image whose units hold `unit` (uniform over the workgroup)
    while (a < b) { const int mid = (a + b + 1) >> 1; if (first[mid] <= unit) a = mid; else b = mid - 1; }
    const SqzImg im = imgs[a];
    uint32_t lw = im.w, lh = im.h;
    for (int l = 0; l < level; ++l) { lw = (lw + 1u) >> 1; lh = (lh + 1u) >> 1; }
    const uint32_t tiles_x = (lw + kTW - 1) / kTW, tiles_y = (lh + kTH - 1) / kTH;
    uint32_t local = unit - first[a];
    const uint32_t plane0 = FINAL ? 0u : local / (tiles_x * tiles_y);
    local -= plane0 * tiles_x * tiles_y;
    const uint32_t x0 = (local % tiles_x) * kTW, y0 = (local / tiles_x) * kTH, i0 = x0 >> 1;
    const uint32_t half_w = lw >> 1, hs = (lw + 1u) >> 1, wl = half_w - 1u;      // high / low counts of a row; the reference's `w`
    const bool odd_w = lw & 1u, from_below = level + 1 < (int)im.levels;        // the LL quarter comes from the level below's output
    const int16_t* below = ((level + 1) & 1) ? scratch1 : scratch0;
    int16_t* mine = (level & 1) ? scratch1 : scratch0;
    const uint64_t row_stride = (uint64_t)im.w << level, plane_elems = (uint64_t)im.w * im.h;
    if (FINAL && im.mode == 2) for (uint32_t k = tid; k < 512u; k += kThreads) table[k] = table_g[k];

    const uint32_t planes = FINAL ? im.planes : 1u;
    for (uint32_t pp = 0; pp < planes; ++pp) {
        const uint32_t plane = plane0 + pp;
        const int16_t* src = coeffs + im.coeff_off + plane * plane_elems;
        const int16_t* ll = below + im.scratch_off + (uint64_t)plane * im.slot;
        if (pp) __syncthreads();                                    // the last plane's readers are through
        // ---- the tile with its halo: rows y0 - 1 .. y0 + kTH + 1 (mirrored), low columns i0 .. i0 + 64, high columns i0 - 1 .. i0 + 64
        for (uint32_t k = tid; k < (uint32_t)(kRows * (kNL + kNH)); k += kThreads) {
            const uint32_t r = k / (kNL + kNH), j = k - r * (kNL + kNH);
            const uint32_t y = (uint32_t)mirror((int)y0 - 1 + (int)r, (int)lh - 1);
            int v = 0;
            if (j < (uint32_t)kNL) {
                const uint32_t i = i0 + j;
                if (i < hs) v = (from_below && !(y & 1u)) ? ll[(uint64_t)(y >> 1) * hs + i] : sm_to_int(src[y * row_stride + i]);
                lo[r][j] = (int16_t)v;
            } else {
                const int i = (int)i0 - 1 + (int)(j - kNL);
                if (i >= 0 && (uint32_t)i < half_w) v = sm_to_int(src[y * row_stride + hs + (uint32_t)i]);
                hi[r][j - kNL] = (int16_t)v;
            }
        }
        __syncthreads();
        // ---- vertical lifting, :1751-1760: even rows from the original odd rows, then odd rows from the updated even rows
        for (int step = 0; step < 2; ++step) {
            const uint32_t nrows = step == 0 ? kTH / 2 + 1 : kTH / 2;   // even rows y0 .. y0 + kTH (slots 1, 3, ..), odd rows y0 + 1 .. y0 + kTH - 1 (slots 2, 4, ..)
            for (uint32_t k = tid; k < nrows * (uint32_t)(kNL + kNH); k += kThreads) {
                const uint32_t q = k / (kNL + kNH), j = k - q * (kNL + kNH), r = 2u * q + 1u + (uint32_t)step;
                int16_t* col = j < (uint32_t)kNL ? &lo[0][j] : &hi[0][j - kNL];
                const uint32_t pitch = j < (uint32_t)kNL ? kNL + 1 : kNH;
                const int up = col[(r - 1) * pitch], dn = col[(r + 1) * pitch], v = col[r * pitch];
                col[r * pitch] = step == 0 ? (int16_t)(v - ((up + dn + 2) >> 2)) : (int16_t)(v + ((up + dn) >> 1));
            }
            __syncthreads();
        }
        // ---- horizontal pass :1699-1741, a pair of outputs (2i, 2i + 1) per step
        for (uint32_t k = tid; k < (uint32_t)(kTH * kTW / 2); k += kThreads) {
            const uint32_t ry = k / (kTW / 2), j = k - ry * (kTW / 2), i = i0 + j, y = y0 + ry;
            if (y >= lh || 2u * i >= lw) continue;
            const int16_t* L = &lo[ry + 1][0];                      // L[j] is column i0 + j
            const int16_t* H = &hi[ry + 1][1];                      // H[j] is high column i0 + j (H[-1]: i0 - 1)
            auto e_int = [&](uint32_t jj) -> int {                  // the int the reference holds for evens[i0 + jj]
                const uint32_t ii = i0 + jj;
                if (ii == 0u) return L[jj] - ((H[jj] + 1) >> 1);
                if (ii <= wl) return L[jj] - ((H[(int)jj - 1] + H[jj] + 2) >> 2);
                return L[jj] - ((H[(int)jj - 1] + 1) >> 1);         // ii == wl + 1, odd width only
            };
            const int e0 = e_int(j);
            int16_t ev = (int16_t)e0, od = 0;
            const bool has_odd = i < half_w;
            if (has_odd) {
                if (i == wl && !odd_w) od = (int16_t)(H[j] + (int)ev);
                else {
                    const int e1 = e_int(j + 1);
                    const int sum = i + 2u <= wl ? e0 + e1 : (int)(int16_t)e0 + (int)(int16_t)e1;     // loop: ints; tail: the shorts read back
                    od = (int16_t)(H[j] - ((-sum) >> 1));
                }
            }
            if constexpr (FINAL) {
                pix[pp][ry][2 * j] = ev;
                if (has_odd) pix[pp][ry][2 * j + 1] = od;
            } else {
                int16_t* d = mine + im.scratch_off + (uint64_t)plane * im.slot + (uint64_t)y * lw + 2u * i;
                if (has_odd && ((uintptr_t)d & 3u) == 0) *reinterpret_cast<uint32_t*>(d) = (uint32_t)(uint16_t)ev | (uint32_t)(uint16_t)od << 16;
                else { d[0] = ev; if (has_odd) d[1] = od; }
            }
        }
    }
    if constexpr (FINAL) {
    __syncthreads();
    // ---- colour: four pixels per step, dword stores where the address allows
    const uint32_t np = im.planes;
    for (uint32_t k = tid; k < (uint32_t)(kTH * kTW / 4); k += kThreads) {
        const uint32_t ry = k / (kTW / 4), xq = (k - ry * (kTW / 4)) * 4u, y = y0 + ry, x = x0 + xq;
        if (y >= lh || x >= lw) continue;
        const uint32_t cnt = min(4u, lw - x);
        uint32_t px[4];
        #pragma unroll
        for (uint32_t t = 0; t < 4u; ++t) px[t] = t < cnt ? colour(im.mode, pix[0][ry][xq + t], pix[1][ry][xq + t], pix[2][ry][xq + t], table) : 0u;
        uint8_t* d = out + im.out_off + ((uint64_t)y * lw + x) * np;
        if (cnt == 4u && ((uintptr_t)d & 3u) == 0) {
            uint32_t* d32 = reinterpret_cast<uint32_t*>(d);
            if (np == 1u) d32[0] = px[0] | px[1] << 8 | px[2] << 16 | px[3] << 24;
            else { d32[0] = px[0] | px[1] << 24; d32[1] = px[1] >> 8 | px[2] << 16; d32[2] = px[2] >> 16 | px[3] << 8; }
        } else {
            for (uint32_t t = 0; t < cnt; ++t) for (uint32_t c = 0; c < np; ++c) d[t * np + c] = (uint8_t)(px[t] >> (8 * c));
        }
    }
    }
}

thread_local float t_stage_ms[3] = { -1.0f, -1.0f, -1.0f };

// descs[i] for i in which[]: validated already.  Queues the upload of the tables and the launches on `stream`, then waits.
int reconstruct(const int16_t* coeffs, const gamut_hip_sqz_desc* descs, const int64_t* out_offset, const std::vector<int>& which, uint8_t* out, hipStream_t stream)
{
    const size_t n = which.size();
    if (!n) return GAMUT_HIP_OK;
    std::vector<SqzImg> imgs(n);
    int max_levels = 0;
    uint64_t scratch_elems = 0;
    for (size_t k = 0; k < n; ++k) {
        const gamut_hip_sqz_desc& d = descs[which[k]];
        SqzImg& im = imgs[k];
        im = SqzImg{};
        im.out_off = out_offset[which[k]]; im.coeff_off = d.coeff_offset;
        im.w = (uint32_t)d.width; im.h = (uint32_t)d.height; im.levels = (uint8_t)d.levels; im.mode = (uint8_t)d.color_mode; im.planes = d.color_mode == 0 ? 1 : 3;
        im.slot = ((im.w + 1u) >> 1) * ((im.h + 1u) >> 1);
        im.scratch_off = (int64_t)scratch_elems;
        if (im.levels > 1) scratch_elems += (uint64_t)im.slot * im.planes;
        max_levels = std::max(max_levels, (int)im.levels);
    }
    // unit tables: per level n + 1 prefix sums
    const size_t tab = n + 1;
    std::vector<uint32_t> first((size_t)max_levels * tab);
    for (int level = 0; level < max_levels; ++level) {
        uint64_t units = 0;
        for (size_t k = 0; k < n; ++k) {
            first[(size_t)level * tab + k] = (uint32_t)units;
            const SqzImg& im = imgs[k];
            if (level < (int)im.levels) {
                uint32_t lw = im.w, lh = im.h;
                for (int l = 0; l < level; ++l) { lw = (lw + 1u) >> 1; lh = (lh + 1u) >> 1; }
                units += (uint64_t)((lw + kTW - 1) / kTW) * ((lh + kTH - 1) / kTH) * (level == 0 ? 1u : im.planes);
            }
            if (units > 0x7FFFFFFFull) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_reconstruct: batch of more than 2^31 - 1 tiles");
        }
        first[(size_t)level * tab + n] = (uint32_t)units;
    }
    const size_t o_first = up256(n * sizeof(SqzImg)), o_table = o_first + up256(first.size() * 4), total = o_table + 512;
    static thread_local PerDevice<DeviceScratch> blob_pd, work_pd;
    static thread_local PerDevice<PinnedScratch> pinned_pd;
    uint8_t* d = (uint8_t*)blob_pd.cur().get(total, stream);
    uint8_t* h = pinned_pd.cur().get(total, stream);
    int16_t* work = (int16_t*)work_pd.cur().get((size_t)(scratch_elems * 2 + 8) * sizeof(int16_t), stream);
    if (!d || !h || !work) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_reconstruct: %zu bytes of tables and %llu bytes of level scratch could not be had", total, (unsigned long long)scratch_elems * 4);
    memset(h, 0, total);
    memcpy(h, imgs.data(), n * sizeof(SqzImg));
    memcpy(h + o_first, first.data(), first.size() * 4);
    memcpy(h + o_table, sqz_linear_to_srgb_table(), 512);
    StreamDrain drain;
    GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, stream));
    drain.arm(stream);
    static const bool timing = env_flag("GAMUT_HIP_SQZ_TIMING");
    KernelTimer<2> timer(timing);
    timer.mark(stream);
    const SqzImg* dimgs = (const SqzImg*)d;
    int16_t *s0 = work, *s1 = work + scratch_elems;
    for (int level = max_levels - 1; level >= 0; --level) {
        const uint32_t* f = (const uint32_t*)(d + o_first) + (size_t)level * tab;
        const uint32_t units = first[(size_t)level * tab + n];
        if (!units) continue;
        if (level > 0) hipLaunchKernelGGL(k_sqz_level<false>, dim3(units), dim3(kThreads), 0, stream, dimgs, f, (int)n, level, coeffs, s0, s1, d + o_table, out);
        else hipLaunchKernelGGL(k_sqz_level<true>, dim3(units), dim3(kThreads), 0, stream, dimgs, f, (int)n, level, coeffs, s0, s1, d + o_table, out);
        if (int rc = launch_status("sqz_reconstruct")) return rc;
    }
    timer.mark(stream);
    const hipError_t e = drain.wait();
    if (e != hipSuccess) return set_error(GAMUT_HIP_ERR_HIP, "sqz_reconstruct: %s", hipGetErrorString(e));
    timer.finish(&t_stage_ms[0]);
    return GAMUT_HIP_OK;
}

int reconstruct_batch(const int16_t* coeffs, const gamut_hip_sqz_desc* descs, int count, const int64_t* out_offset, uint8_t* out, int* status_host, hipStream_t stream)
{
    std::vector<int> which;
    int first_bad = -1; char first_msg[200] = { 0 };
    for (int i = 0; i < count; ++i) {
        const gamut_hip_sqz_desc& d = descs[i];
        int rc = GAMUT_HIP_OK;
        if (!sqz_valid_geometry(d.width, d.height, d.color_mode, 0, d.levels)) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: geometry %d x %d, colour mode %d, %d levels is not an SQZ image's", d.width, d.height, d.color_mode, d.levels);
        else if (d.coeff_offset < 0 || out_offset[i] < 0) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: negative offset");
        if (status_host) status_host[i] = rc;
        if (rc == GAMUT_HIP_OK) which.push_back(i);
        else if (first_bad < 0) { first_bad = i; snprintf(first_msg, sizeof(first_msg), "%s", last_error_buf()); }
    }
    if (int rc = reconstruct(coeffs, descs, out_offset, which, out, stream)) return rc;
    if (first_bad >= 0) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "image %d: %s", first_bad, first_msg);
    return GAMUT_HIP_OK;
}

int decode_batch(const uint8_t* const* data, const size_t* len, int count, const int64_t* out_offset, uint8_t* out, gamut_hip_sqz_info* info,
                 int* status_host, hipStream_t stream)
{
    static const bool timing = env_flag("GAMUT_HIP_SQZ_TIMING");
    std::vector<int> good; std::vector<gamut_hip_sqz_desc> descs((size_t)count); std::vector<gamut_hip_sqz_info> hd((size_t)count);
    int first_bad = -1, first_rc = GAMUT_HIP_OK; char first_msg[200] = { 0 };
    auto refuse = [&](int i, int rc, const char* msg) {
        if (status_host) status_host[i] = rc;
        if (first_bad < 0 || i < first_bad) { first_bad = i; first_rc = rc; snprintf(first_msg, sizeof(first_msg), "%s", msg); }
    };
    uint64_t elems = 0;
    for (int i = 0; i < count; ++i) {
        int rc = sqz_parse_header(data[i], len[i], &hd[(size_t)i]);
        if (info) info[i] = hd[(size_t)i];
        if (status_host) status_host[i] = GAMUT_HIP_OK;
        if (rc == GAMUT_HIP_OK && out_offset[i] < 0) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: negative out_offset");
        if (rc != GAMUT_HIP_OK) { refuse(i, rc, last_error_buf()); continue; }
        const gamut_hip_sqz_info& s = hd[(size_t)i];
        descs[(size_t)i] = gamut_hip_sqz_desc{ s.width, s.height, s.color_mode, s.levels, (int64_t)elems };
        elems += (uint64_t)s.width * (uint64_t)s.height * (uint64_t)s.planes;
        elems = (elems + 7u) & ~(uint64_t)7u;                       // every image's planes start at a 16-byte boundary
        good.push_back(i);
    }
    if (!good.empty()) {
        const size_t bytes = (size_t)elems * sizeof(int16_t);
        static thread_local PerDevice<DeviceScratch> coeff_pd;
        static thread_local PerDevice<PinnedScratch> stage_pd;
        int16_t* dco = (int16_t*)coeff_pd.cur().get(bytes, stream);
        if (sqz_reader() == 1) {                                    // the device reader: files up, no coefficient crosses the bus
            if (!dco) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_decode: %zu coefficient bytes could not be had", bytes);
            std::vector<int64_t> coff((size_t)count, 0);
            for (int i : good) coff[(size_t)i] = descs[(size_t)i].coeff_offset;
            if (timing) t_stage_ms[1] = t_stage_ms[2] = -1.0f;
            if (int rc = sqz_read_files(data, len, hd.data(), good, dco, coff.data(), stream)) return rc;
            if (int rc = reconstruct(dco, descs.data(), out_offset, good, out, stream)) return rc;
            if (first_bad >= 0) return set_error(first_rc, "image %d: %s", first_bad, first_msg);
            return GAMUT_HIP_OK;
        }
        int16_t* hco = (int16_t*)stage_pd.cur().get(bytes, stream);
        if (!dco || !hco) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_decode: staging of %zu coefficient bytes failed", bytes);
        // the front end: one file per host thread, straight into the pinned staging
        const TracePoint t0 = trace_now();
        std::vector<int> rcs(good.size(), GAMUT_HIP_OK);
        const int workers = std::min(std::min(host_threads(), 16), (int)good.size());
        parallel_for((int)good.size(), workers, [&](int, int k) {
            const int i = good[(size_t)k];
            gamut_hip_sqz_info s;
            const gamut_hip_sqz_desc& d = descs[(size_t)i];
            int rc;
            try { rc = sqz_decode_coeffs(data[i], len[i], hco + d.coeff_offset, (size_t)d.width * d.height * (d.color_mode == 0 ? 1 : 3), &s); }
            catch (...) { rc = GAMUT_HIP_ERR_OUT_OF_MEMORY; }
            rcs[(size_t)k] = rc;
        });
        if (timing) t_stage_ms[1] = (float)ms_since(t0);
        std::vector<int> run;
        for (size_t k = 0; k < good.size(); ++k) {
            if (rcs[k] == GAMUT_HIP_OK) run.push_back(good[k]);
            else refuse(good[k], rcs[k], "sqz: out of host memory in the front end");
        }
        const TracePoint t1 = trace_now();
        {
            StreamDrain drain;
            GAMUT_HIP_CHECK(hipMemcpyAsync(dco, hco, bytes, hipMemcpyHostToDevice, stream));
            drain.arm(stream);
            if (timing) t_stage_ms[2] = (float)ms_since(t1);
            if (int rc = reconstruct(dco, descs.data(), out_offset, run, out, stream)) return rc;
            const hipError_t e = drain.wait();
            if (e != hipSuccess) return set_error(GAMUT_HIP_ERR_HIP, "sqz_decode: %s", hipGetErrorString(e));
        }
    }
    if (first_bad >= 0) return set_error(first_rc, "image %d: %s", first_bad, first_msg);
    return GAMUT_HIP_OK;
}

} // namespace
} // namespace gamut

using namespace gamut;

extern "C" {

int gamut_hip_sqz_reconstruct_batch_device(const int16_t* coeffs, const gamut_hip_sqz_desc* descs, int count, const int64_t* out_offset,
                                           uint8_t* out, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!coeffs || !descs || !out_offset || !out)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_reconstruct_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return reconstruct_batch(coeffs, descs, count, out_offset, out, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_reconstruct_batch_device: out of host memory");
    }
}

int gamut_hip_sqz_decode_batch_device(const uint8_t* const* data, const size_t* len, int count, const int64_t* out_offset, uint8_t* out,
                                      gamut_hip_sqz_info* info, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!data || !len || !out_offset || !out)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_decode_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return decode_batch(data, len, count, out_offset, out, info, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_decode_batch_device: out of host memory");
    }
}

float gamut_hip_sqz_last_decode_stage_ms(int stage) { return stage >= 0 && stage < 3 ? t_stage_ms[stage] : -1.0f; }

} // extern "C"
