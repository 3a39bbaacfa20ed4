// sqz_encode.hip -- the SQZ front half on the GPU and the calls above it: l8 / rgb8 pixels in HBM -> the reference's coefficient buffer
// as it stands before SQZ_schedule_task, bit for bit what SQZ_color_process(read = 1), SQZ_dwt and SQZ_dwt_convert_to_sign_magnitude
// (source/gamut/codecs/sqz.d:1153-1546, 1597-1697, 1574-1582) make of them.  The back half (the bit-plane writer) is sqz_host.hip on host
// threads or sqz_write.hip on the device, by gamut_hip_sqz_set_writer; the files stay in HBM only with the latter.
//
// THE REFERENCE'S ORDER, AND WHY A LEVEL IS DATA-PARALLEL.  SQZ_dwt_5_3i (:1645-1673) starts with nnn = row 3, nn = row 2 (SQZ_mirror of
// -3 and -2) and walks i = -2, 0, 2, ..: n = row i + 1, r = row i + 2 (mirrored); the horizontal passes of n (if nn <= r) and of r (if
// i + 2 < height); the predict step n -= (nn + r) >> 1 (if nn <= r); the update step nn += (nnn + n + 2) >> 2 (if nnn <= n).
//   i = -2: n = 1, r = 0, nn = 2 > r: only row 0's horizontal pass; nnn = 3 > n: no update.  Then nnn = 1, nn = 0.
//   i = 0:  n = 1, r = 2: horizontal passes of rows 1 and 2; row 1 -= (row 0 + row 2) >> 1, both passed and neither updated; nnn = n
//           = row 1: row 0 += (row 1 + row 1 + 2) >> 2 -- row -1 is row 1.
//   i = 2k: rows 2k + 1 and 2k + 2 are passed, row 2k + 1 is predicted from rows 2k and 2k + 2 (row 2k is updated only AFTER, in this
//           same iteration), row 2k is updated from the predicted rows 2k - 1 and 2k + 1.
//   even height h, i = h - 2: n = h - 1, r = mirror(h) = h - 2 = nn: row h - 1 is passed (r is not: i + 2 = h), predicted from row
//           h - 2 twice (passed in the iteration before as r, not yet updated) -- row h is row h - 2; row h - 2 is updated.  i = h ends.
//   odd height h, i = h - 3: as i = 2k; then i = h - 1: n = mirror(h) = h - 2, r = mirror(h + 1) = h - 3 < nn = h - 1: no pass, no
//           predict; nnn = n = h - 2: row h - 1 += (row h - 2 + row h - 2 + 2) >> 2 -- row h is row h - 2.
// So a level equals: every row's horizontal pass; then every odd row predicted from the passed, not yet updated even rows; then every
// even row updated from the predicted odd rows; rows outside the image by symmetric extension (-1 is 1, h is h - 2).  The vertical
// steps are `short op= int`: they wrap to 16 bits, and they read shorts.
//
// THE HORIZONTAL PASS (:1597-1643) splits a row into evens e(i) and odds o(i) and writes [low half | high half].  With the INT
// H(i) = o(i) + ((-(e(i) + e(i + 1))) >> 1) (the last one of an even width: o - e), hw = width / 2 and w = hw - 1 >= 3:
//   high[i] = (short)H(i);
//   low[0] = e(0) + (((short)H(0) + 1) >> 1)              cf1 is assigned from the cast at i = 0;
//   low[1] = e(1) + (((short)H(0) + H(1) + 2) >> 2)       the truncated cf1 again, the untruncated cf3;
//   low[i] = e(i) + ((H(i - 1) + H(i) + 2) >> 2)          1 < i < w: both running values are ints;
//   low[w] = e(w) + (((short)H(w - 1) + H(w) + 2) >> 2)   the tail reads h_band[w - 1] back as a short, cf3 is an int;
//   low[w + 1] = e(w + 1) + ((H(w) + 1) >> 1)             odd widths only;
// each stored through cast(short).  (When w is even the loop's second half-step runs once more at i = w, reading evens[w + 1] --
// for an even width that is odds[0] in the scratch row -- and the tail overwrites both values it stored.)  H leaves 16 bits when
// o - (e + e') / 2 does; the difference between the two readings is kept.
//
// LAUNCHES.  One per level, SHALLOWEST first, each over every image of the batch that has that level (a table of unit counts per
// image, binary search per workgroup -- the scheme of k_sqz_level): at most eight.  A workgroup takes a 128 x 16 tile of the level's
// INPUT with a halo of two samples on every side (a low output reads five inputs, a high one three) into LDS, does the horizontal
// pass of its 19 rows, the two vertical steps, and stores: the three detail bands to their interleaved places in the caller's
// buffer, converted to sign-magnitude in the store; the LL quarter compact into one of two scratch buffers used alternately, where the
// next level reads it (tiling rules out working in place); the deepest level's LL into the caller's buffer as well.  Level 0 takes
// one unit per tile for ALL planes: the colour transform sits in its load and is done once per pixel and tile.
#include "common.hpp"
#include "encode_host.hpp"
#include "sqz_write.hpp"

namespace gamut {
const uint16_t* sqz_srgb_to_linear_table();                                                      // sqz_host.hip
namespace {

constexpr int kThreads = 256, kTW = 128, kTH = 16, kRows = kTH + 3, kCols = kTW + 3, kHalf = kTW / 2;

struct FwdImg {
    const uint8_t* src; int64_t pitch;                              // level 0 reads pixels (bytes, rows `pitch` apart) or int16 planes (from_planes)
    int64_t coeff_off, scratch_off;                                 // int16 elements; int16 elements inside either scratch buffer
    uint32_t w, h, slot;                                            // slot: elements of one plane in a scratch buffer = ceil(w / 2) * ceil(h / 2)
    uint8_t levels, mode, planes, from_planes;
};

__device__ __forceinline__ int mirror(int v, int maximum)           // SQZ_mirror :513-526, maximum >= 7
{
    while ((uint32_t)v > (uint32_t)maximum) { v = -v; if (v < 0) v += 2 * maximum; }
    return v;
}
__device__ __forceinline__ int16_t to_sm(int16_t v) { const int x = v; return (int16_t)(x < 0 ? (-2 * x) | 1 : 2 * x); }     // :1580
__device__ __forceinline__ int cbrt01(int v)                        // SQZ_i32_cbrt_01 :1368-1385
{
    if (v <= 0) return 0;
    if (v >= 65535) return 65535;
    int64_t root = ((v * (((v * (v - 144107LL)) >> 16) + 132114LL)) >> 16) + 14379LL;
    #pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int64_t n = root * root * root, den = v + (n >> 31);
        root = (root * (2LL * v + (n >> 32))) / den;
    }
    return (int)root;
}
// one pixel -> the three planes' values (grey: c[0] alone), SQZ_color_process_* with read = 1
__device__ __forceinline__ void colour(int mode, int R, int G, int B, const uint16_t* s2l, int16_t c[3])
{
    if (mode == 0) { c[0] = (int16_t)(R - 128); return; }                                           // :1167
    if (mode == 1) {                                                                                // YCoCg-R :1205-1211
        const int16_t t = (int16_t)((R + B) >> 1);
        c[0] = (int16_t)(((t + G) >> 1) - 128); c[1] = (int16_t)(R - B); c[2] = (int16_t)(G - t);
    } else if (mode == 2) {                                                                         // Oklab :1408-1416
        const int64_t r = s2l[R], g = s2l[G], b = s2l[B];
        const int64_t l = cbrt01((int)((27015LL * r + 35149LL * g + 3372LL * b) >> 16));
        const int64_t m = cbrt01((int)((13887LL * r + 44610LL * g + 7038LL * b) >> 16));
        const int64_t s = cbrt01((int)((5787LL * r + 18462LL * g + 41286LL * b) >> 16));
        c[0] = (int16_t)(((862LL * l + 3250LL * m - 17LL * s + 32767) >> 16) - 2048);
        c[1] = (int16_t)((8100LL * l - 9945LL * m + 1845LL * s + 32767) >> 16);
        c[2] = (int16_t)((106LL * l + 3205LL * m - 3311LL * s + 32767) >> 16);
    } else {                                                                                        // LOG-L1 :1486-1491, 32 bits
        c[0] = (int16_t)(((33779 * R + 41184 * G + 38182 * B) >> 16) - 221);
        c[1] = (int16_t)((-52830 * R + 8188 * G + 37906 * B) >> 16);
        c[2] = (int16_t)((19051 * R - 50317 * G + 37420 * B) >> 16);
    }
}

// Level `level` of the batch.  first[i] .. first[i + 1]: the units (workgroups) of image i; FIRST (level 0): one unit per tile, the colour
// stage (or the caller's planes) in the load, all planes; otherwise one unit per plane and tile, read from scratch[(level - 1) & 1].
template <bool FIRST>
__global__ __launch_bounds__(kThreads) void k_sqz_forward(const FwdImg* __restrict__ imgs, const uint32_t* __restrict__ first, int count, int level,
                                                          int16_t* __restrict__ coeffs, int16_t* __restrict__ scratch0, int16_t* __restrict__ scratch1,
                                                          const uint16_t* __restrict__ table_g)
{
    __shared__ int16_t in[FIRST ? 3 : 1][kRows][kCols + 1];
    __shared__ int16_t lo[kRows][kHalf];
    __shared__ int16_t hi[kRows][kHalf];
    __shared__ uint16_t s2l[FIRST ? 256 : 2];
    const uint32_t tid = threadIdx.x, unit = blockIdx.x;
    int a = 0, b = count - 1;                                       // the image whose units hold `unit` (uniform over the workgroup)
    while (a < b) { const int mid = (a + b + 1) >> 1; if (first[mid] <= unit) a = mid; else b = mid - 1; }
    const FwdImg im = imgs[a];
    uint32_t lw = im.w, lh = im.h;
    for (int l = 0; l < level; ++l) { lw = (lw + 1u) >> 1; lh = (lh + 1u) >> 1; }
    const uint32_t tiles_x = (lw + kTW - 1) / kTW, tiles_y = (lh + kTH - 1) / kTH;
    uint32_t local = unit - first[a];
    const uint32_t plane0 = FIRST ? 0u : local / (tiles_x * tiles_y);
    local -= plane0 * tiles_x * tiles_y;
    const uint32_t x0 = (local % tiles_x) * kTW, y0 = (local / tiles_x) * kTH, i0 = x0 >> 1;
    const uint32_t half_w = lw >> 1, hs = (lw + 1u) >> 1, wl = half_w - 1u;      // high / low counts of a row; the reference's `w`
    const bool odd_w = lw & 1u, last_level = level + 1 == (int)im.levels;
    const int16_t* below = ((level + 1) & 1) ? scratch1 : scratch0;
    int16_t* mine = (level & 1) ? scratch1 : scratch0;
    const uint64_t row_stride = (uint64_t)im.w << level, plane_elems = (uint64_t)im.w * im.h;
    const uint32_t planes = FIRST ? im.planes : 1u;

    // ---- the tile with its halo: rows y0 - 2 .. y0 + kTH (mirrored), columns x0 - 2 .. x0 + kTW (zero outside the row: not used)
    if constexpr (FIRST) {
        if (im.mode == 2 && !im.from_planes) {
            for (uint32_t k = tid; k < 256u; k += kThreads) s2l[k] = table_g[k];
            __syncthreads();
        }
        for (uint32_t k = tid; k < (uint32_t)(kRows * kCols); k += kThreads) {
            const uint32_t r = k / kCols, j = k - r * kCols;
            const uint32_t y = (uint32_t)mirror((int)y0 - 2 + (int)r, (int)lh - 1);
            const int x = (int)x0 - 2 + (int)j;
            int16_t c[3] = { 0, 0, 0 };
            if (x >= 0 && (uint32_t)x < lw) {
                if (im.from_planes) {
                    const int16_t* p = reinterpret_cast<const int16_t*>(im.src) + (uint64_t)y * lw + (uint32_t)x;
                    for (uint32_t pp = 0; pp < planes; ++pp) c[pp] = p[pp * plane_elems];
                } else {
                    const uint8_t* p = im.src + (int64_t)y * im.pitch + (int64_t)x * planes;
                    if (planes == 1u) colour(0, p[0], 0, 0, s2l, c);
                    else colour(im.mode, p[0], p[1], p[2], s2l, c);
                }
            }
            for (uint32_t pp = 0; pp < planes; ++pp) in[pp][r][j] = c[pp];
        }
    } else {
        const int16_t* ll = below + im.scratch_off + (uint64_t)plane0 * im.slot;
        for (uint32_t k = tid; k < (uint32_t)(kRows * kCols); k += kThreads) {
            const uint32_t r = k / kCols, j = k - r * kCols;
            const uint32_t y = (uint32_t)mirror((int)y0 - 2 + (int)r, (int)lh - 1);
            const int x = (int)x0 - 2 + (int)j;
            in[0][r][j] = (x >= 0 && (uint32_t)x < lw) ? ll[(uint64_t)y * lw + (uint32_t)x] : (int16_t)0;
        }
    }
    __syncthreads();

    for (uint32_t pp = 0; pp < planes; ++pp) {
        const uint32_t plane = plane0 + pp;
        if (pp) __syncthreads();                                    // the last plane's stores have read lo / hi
        // ---- horizontal pass :1597-1643: low and high output i0 + j of every row of the tile
        for (uint32_t k = tid; k < (uint32_t)(kRows * kHalf); k += kThreads) {
            const uint32_t r = k / kHalf, j = k - r * kHalf, i = i0 + j;
            const int16_t* row = &in[pp][r][2u * j + 2u];           // row[0] = e(i), row[1] = o(i), row[2] = e(i + 1); row[-2], row[-1]: e(i - 1), o(i - 1)
            int L = 0, H = 0;
            if (i < hs) {
                const int e = row[0];
                auto h_int = [&](int d) -> int {                    // the int H(i + d), d = -1 or 0, i + d < half_w
                    const int16_t* q = row + 2 * d;
                    return (i + d == wl && !odd_w) ? q[1] - q[0] : q[1] + ((-(q[0] + q[2])) >> 1);
                };
                if (i < half_w) H = h_int(0);
                if (i == 0u) L = e + (((int)(int16_t)H + 1) >> 1);
                else if (i > wl) L = e + ((h_int(-1) + 1) >> 1);   // i = w + 1, odd widths
                else {
                    int hp = h_int(-1);
                    if (i == 1u || i == wl) hp = (int16_t)hp;      // cf1 assigned from the cast; h_band[w - 1] read back
                    L = e + ((hp + H + 2) >> 2);
                }
            }
            lo[r][j] = (int16_t)L;
            hi[r][j] = (int16_t)H;
        }
        __syncthreads();
        // ---- vertical steps :1660-1669: odd rows (slots 1, 3, .., 17) from the passed even rows, then even rows (slots 2, .., 16) from those
        for (int step = 0; step < 2; ++step) {
            const uint32_t nrows = step == 0 ? kTH / 2 + 1 : kTH / 2;
            for (uint32_t k = tid; k < nrows * (uint32_t)kTW; k += kThreads) {
                const uint32_t q = k / kTW, j = k - q * kTW, r = 2u * q + 1u + (uint32_t)step;
                int16_t* col = j < (uint32_t)kHalf ? &lo[0][j] : &hi[0][j - kHalf];
                const int up = col[(r - 1) * kHalf], dn = col[(r + 1) * kHalf], v = col[r * kHalf];
                col[r * kHalf] = step == 0 ? (int16_t)(v - ((up + dn) >> 1)) : (int16_t)(v + ((up + dn + 2) >> 2));
            }
            __syncthreads();
        }
        // ---- stores: rows y0 .. y0 + kTH - 1 are slots 2 .. kTH + 1
        int16_t* dst = coeffs + im.coeff_off + plane * plane_elems;
        int16_t* ll_out = mine + im.scratch_off + (uint64_t)plane * im.slot;
        for (uint32_t k = tid; k < (uint32_t)(kTH * kTW); k += kThreads) {
            const uint32_t ry = k / kTW, j = k - ry * kTW, y = y0 + ry;
            const bool high = j >= (uint32_t)kHalf;
            const uint32_t i = i0 + (high ? j - kHalf : j);
            if (y >= lh || i >= (high ? half_w : hs)) continue;
            const int16_t v = high ? hi[ry + 2][j - kHalf] : lo[ry + 2][j];
            if (!high && !(y & 1u) && !last_level) ll_out[(uint64_t)(y >> 1) * hs + i] = v;
            else dst[(uint64_t)y * row_stride + (high ? hs + i : i)] = to_sm(v);
        }
    }
}

thread_local float t_stage_ms[3] = { -1.0f, -1.0f, -1.0f };

struct Source { const uint8_t* ptr; int64_t pitch; bool planes; };

// descs[i] for i in which[]: checked and clamped already.  Queues the upload of the tables and the launches on `stream`, then waits.
int forward(const std::vector<Source>& src, const gamut_hip_sqz_encode_desc* descs, const int64_t* coeff_offset, const std::vector<int>& which,
            int16_t* coeffs, hipStream_t stream)
{
    const size_t n = which.size();
    if (!n) return GAMUT_HIP_OK;
    std::vector<FwdImg> imgs(n);
    int max_levels = 0;
    uint64_t scratch_elems = 0;
    for (size_t k = 0; k < n; ++k) {
        const gamut_hip_sqz_encode_desc& d = descs[which[k]];
        FwdImg& im = imgs[k];
        im = FwdImg{};
        im.src = src[(size_t)which[k]].ptr; im.pitch = src[(size_t)which[k]].pitch; im.from_planes = src[(size_t)which[k]].planes;
        im.coeff_off = coeff_offset[which[k]];
        im.w = (uint32_t)d.width; im.h = (uint32_t)d.height; im.levels = (uint8_t)d.levels; im.mode = (uint8_t)d.color_mode; im.planes = d.color_mode == 0 ? 1 : 3;
        im.slot = ((im.w + 1u) >> 1) * ((im.h + 1u) >> 1);
        im.scratch_off = (int64_t)scratch_elems;
        if (im.levels > 1) scratch_elems += (uint64_t)im.slot * im.planes;
        max_levels = std::max(max_levels, (int)im.levels);
    }
    const size_t tab = n + 1;                                       // unit tables: per level n + 1 prefix sums
    std::vector<uint32_t> first((size_t)max_levels * tab);
    for (int level = 0; level < max_levels; ++level) {
        uint64_t units = 0;
        for (size_t k = 0; k < n; ++k) {
            first[(size_t)level * tab + k] = (uint32_t)units;
            const FwdImg& im = imgs[k];
            if (level < (int)im.levels) {
                uint32_t lw = im.w, lh = im.h;
                for (int l = 0; l < level; ++l) { lw = (lw + 1u) >> 1; lh = (lh + 1u) >> 1; }
                units += (uint64_t)((lw + kTW - 1) / kTW) * ((lh + kTH - 1) / kTH) * (level == 0 ? 1u : im.planes);
            }
            if (units > 0x7FFFFFFFull) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_analyze: batch of more than 2^31 - 1 tiles");
        }
        first[(size_t)level * tab + n] = (uint32_t)units;
    }
    const size_t o_first = up256(n * sizeof(FwdImg)), o_table = o_first + up256(first.size() * 4), total = o_table + 512;
    static thread_local PerDevice<DeviceScratch> blob_pd, work_pd;
    static thread_local PerDevice<PinnedScratch> pinned_pd;
    uint8_t* d = (uint8_t*)blob_pd.cur().get(total, stream);
    uint8_t* h = pinned_pd.cur().get(total, stream);
    int16_t* work = (int16_t*)work_pd.cur().get((size_t)(scratch_elems * 2 + 8) * sizeof(int16_t), stream);
    if (!d || !h || !work) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_analyze: %zu bytes of tables and %llu bytes of level scratch could not be had", total, (unsigned long long)scratch_elems * 4);
    memset(h, 0, total);
    memcpy(h, imgs.data(), n * sizeof(FwdImg));
    memcpy(h + o_first, first.data(), first.size() * 4);
    memcpy(h + o_table, sqz_srgb_to_linear_table(), 512);
    StreamDrain drain;
    GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, stream));
    drain.arm(stream);
    static const bool timing = env_flag("GAMUT_HIP_SQZ_TIMING");
    KernelTimer<2> timer(timing);
    timer.mark(stream);
    const FwdImg* dimgs = (const FwdImg*)d;
    int16_t *s0 = work, *s1 = work + scratch_elems;
    for (int level = 0; level < max_levels; ++level) {
        const uint32_t* f = (const uint32_t*)(d + o_first) + (size_t)level * tab;
        const uint32_t units = first[(size_t)level * tab + n];
        if (!units) continue;
        if (level == 0) hipLaunchKernelGGL(k_sqz_forward<true>, dim3(units), dim3(kThreads), 0, stream, dimgs, f, (int)n, level, coeffs, s0, s1, (const uint16_t*)(d + o_table));
        else hipLaunchKernelGGL(k_sqz_forward<false>, dim3(units), dim3(kThreads), 0, stream, dimgs, f, (int)n, level, coeffs, s0, s1, (const uint16_t*)(d + o_table));
        if (int rc = launch_status("sqz_analyze")) return rc;
    }
    timer.mark(stream);
    const hipError_t e = drain.wait();
    if (e != hipSuccess) return set_error(GAMUT_HIP_ERR_HIP, "sqz_analyze: %s", hipGetErrorString(e));
    timer.finish(&t_stage_ms[0]);
    return GAMUT_HIP_OK;
}

using Refusals = SqzRefusals;                                       // sqz_write.hpp

// Which back half the file-level calls run: 0 the host writer (sqz_host.hip), 1 the device writer (sqz_write.hip)
std::atomic<int>& writer_switch()
{
    static std::atomic<int> w{ [] { const char* e = getenv("GAMUT_HIP_SQZ_WRITER"); return e && !strcmp(e, "device") ? 1 : 0; }() };
    return w;
}

int analyze_batch(const uint8_t* const* src, const int64_t* src_pitch, const int16_t* planes_in, const gamut_hip_sqz_encode_desc* descs, int count,
                  int16_t* coeffs, const int64_t* coeff_offset, int* status_host, hipStream_t stream)
{
    std::vector<gamut_hip_sqz_encode_desc> checked(descs, descs + count);
    std::vector<Source> sources((size_t)count);
    std::vector<int> which;
    Refusals bad; bad.status = status_host;
    for (int i = 0; i < count; ++i) {
        if (status_host) status_host[i] = GAMUT_HIP_OK;
        int rc = sqz_encode_check(&checked[(size_t)i]);
        if (rc == GAMUT_HIP_OK && coeff_offset[i] < 0) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: negative coeff_offset");
        if (rc == GAMUT_HIP_OK && !planes_in && !src[i]) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: src is NULL");
        if (rc != GAMUT_HIP_OK) { bad.refuse(i, rc); continue; }
        sources[(size_t)i] = planes_in ? Source{ reinterpret_cast<const uint8_t*>(planes_in + coeff_offset[i]), 0, true } : Source{ src[i], src_pitch[i], false };
        which.push_back(i);
    }
    if (int rc = forward(sources, checked.data(), coeff_offset, which, coeffs, stream)) return rc;
    return bad.verdict();
}

// out_on_device: the files stay in HBM, which only the device writer can do; a host `out` gets the writer the switch names
int encode_batch(const uint8_t* const* src, const int64_t* src_pitch, const gamut_hip_sqz_encode_desc* descs, int count, const int64_t* out_offset,
                 uint8_t* out, int64_t* out_len, int* status_host, hipStream_t stream, bool out_on_device = false)
{
    const bool device_writer = out_on_device || writer_switch().load(std::memory_order_relaxed) == 1;
    static const bool timing = env_flag("GAMUT_HIP_SQZ_TIMING");
    std::vector<gamut_hip_sqz_encode_desc> checked(descs, descs + count);
    std::vector<Source> sources((size_t)count);
    std::vector<int64_t> offs((size_t)count, 0);
    std::vector<int> which;
    Refusals bad; bad.status = status_host;
    uint64_t elems = 0;
    for (int i = 0; i < count; ++i) {
        if (status_host) status_host[i] = GAMUT_HIP_OK;
        out_len[i] = 0;
        gamut_hip_sqz_encode_desc& d = checked[(size_t)i];
        int rc = sqz_encode_check(&d);
        if (rc == GAMUT_HIP_OK && d.budget <= 6) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: a budget of %lld bytes does not hold the 6-byte header and one more bit", (long long)d.budget);
        if (rc == GAMUT_HIP_OK && out_offset[i] < 0) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: negative out_offset");
        if (rc == GAMUT_HIP_OK && !src[i]) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: src is NULL");
        if (rc != GAMUT_HIP_OK) { bad.refuse(i, rc); continue; }
        sources[(size_t)i] = Source{ src[i], src_pitch[i], false };
        offs[(size_t)i] = (int64_t)elems;
        elems += (uint64_t)d.width * (uint64_t)d.height * (d.color_mode == 0 ? 1u : 3u);
        elems = (elems + 7u) & ~(uint64_t)7u;                       // every image's planes start at a 16-byte boundary
        which.push_back(i);
    }
    if (!which.empty()) {
        const size_t bytes = (size_t)elems * sizeof(int16_t);
        static thread_local PerDevice<DeviceScratch> coeff_pd;
        static thread_local PerDevice<PinnedScratch> stage_pd;
        int16_t* dco = (int16_t*)coeff_pd.cur().get(bytes, stream);
        int16_t* hco = device_writer ? nullptr : (int16_t*)stage_pd.cur().get(bytes, stream);
        if (!dco || (!hco && !device_writer)) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_encode: staging of %zu coefficient bytes failed", bytes);
        if (int rc = forward(sources, checked.data(), offs.data(), which, dco, stream)) return rc;
        if (device_writer) {                                        // no coefficient leaves HBM; stages 1 and 2 do not exist (gamut_hip_sqz_last_write_stage_ms has the writer's)
            if (timing) t_stage_ms[1] = t_stage_ms[2] = -1.0f;
            std::vector<int> rcs;
            if (int rc = sqz_write_files(dco, offs.data(), checked.data(), which, out_offset, out, out_on_device, out_len, rcs, stream)) return rc;
            for (size_t k = 0; k < which.size(); ++k)
                if (rcs[k] != GAMUT_HIP_OK) { sqz_undefined_shift_error(); bad.refuse(which[k], rcs[k]); }
            return bad.verdict();
        }
        const TracePoint t0 = trace_now();
        {
            StreamDrain drain;
            GAMUT_HIP_CHECK(hipMemcpyAsync(hco, dco, bytes, hipMemcpyDeviceToHost, stream));
            drain.arm(stream);
            const hipError_t e = drain.wait();
            if (e != hipSuccess) return set_error(GAMUT_HIP_ERR_HIP, "sqz_encode: %s", hipGetErrorString(e));
        }
        if (timing) t_stage_ms[2] = (float)ms_since(t0);
        // the back half: one image per host thread.  The writer wants its whole budget zeroed; only the used bytes may reach `out`
        const TracePoint t1 = trace_now();
        std::vector<int> rcs(which.size(), GAMUT_HIP_OK);
        std::vector<std::string> msgs(which.size());
        const int workers = std::min(std::min(host_threads(), 16), (int)which.size());
        parallel_for((int)which.size(), workers, [&](int, int k) {
            const int i = which[(size_t)k];
            const gamut_hip_sqz_encode_desc& d = checked[(size_t)i];
            int rc; int64_t n = 0;
            try {
                std::unique_ptr<uint8_t[]> file(new uint8_t[(size_t)d.budget]);
                rc = sqz_encode_coeffs(hco + offs[(size_t)i], d, file.get(), &n);
                if (rc == GAMUT_HIP_OK) memcpy(out + out_offset[i], file.get(), (size_t)n);
                else msgs[(size_t)k] = last_error_buf();
            } catch (...) { rc = GAMUT_HIP_ERR_OUT_OF_MEMORY; msgs[(size_t)k] = "sqz: out of host memory in the writer"; }
            rcs[(size_t)k] = rc;
            out_len[i] = rc == GAMUT_HIP_OK ? n : 0;
        });
        if (timing) t_stage_ms[1] = (float)ms_since(t1);
        for (size_t k = 0; k < which.size(); ++k)
            if (rcs[k] != GAMUT_HIP_OK) { set_error(rcs[k], "%s", msgs[k].c_str()); bad.refuse(which[k], rcs[k]); }
    }
    return bad.verdict();
}

} // namespace
} // namespace gamut

using namespace gamut;

extern "C" {

int gamut_hip_sqz_analyze_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const gamut_hip_sqz_encode_desc* descs, int count,
                                       int16_t* coeffs, const int64_t* coeff_offset, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!src || !src_pitch || !descs || !coeffs || !coeff_offset)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_analyze_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return analyze_batch(src, src_pitch, nullptr, descs, count, coeffs, coeff_offset, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_analyze_batch_device: out of host memory");
    }
}

int gamut_hip_sqz_dwt_batch_device(const int16_t* planes_in, const gamut_hip_sqz_encode_desc* descs, int count, int16_t* coeffs,
                                   const int64_t* coeff_offset, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!planes_in || !descs || !coeffs || !coeff_offset || planes_in == coeffs)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_dwt_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return analyze_batch(nullptr, nullptr, planes_in, descs, count, coeffs, coeff_offset, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_dwt_batch_device: out of host memory");
    }
}

int gamut_hip_sqz_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const gamut_hip_sqz_encode_desc* descs, int count,
                                      const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!src || !src_pitch || !descs || !out_offset || !out || !out_len)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_encode_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return encode_batch(src, src_pitch, descs, count, out_offset, out, out_len, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_encode_batch_device: out of host memory");
    }
}

int gamut_hip_sqz_encode_batch_to_device(const uint8_t* const* src, const int64_t* src_pitch, const gamut_hip_sqz_encode_desc* descs, int count,
                                         const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!src || !src_pitch || !descs || !out_offset || !out || !out_len)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_encode_batch_to_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return encode_batch(src, src_pitch, descs, count, out_offset, out, out_len, status_host, pick_stream(stream), true);
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_encode_batch_to_device: out of host memory");
    }
}

int gamut_hip_sqz_set_writer(int which)
{
    if (which != 0 && which != 1) return writer_switch().load(std::memory_order_relaxed);
    return writer_switch().exchange(which, std::memory_order_relaxed);
}

void* gamut_hip_sqz_write_to_mem(const void* data, int pitch, const gamut_hip_sqz_encode_desc* desc, int* out_len)
{
    clear_error();
    if (out_len) *out_len = 0;
    if (!data || !desc || !out_len) { set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_write_to_mem: invalid arguments"); return nullptr; }
    gamut_hip_sqz_encode_desc d = *desc;
    if (sqz_encode_check(&d) != GAMUT_HIP_OK) return nullptr;
    if (d.budget <= 6 || d.budget > 0x7FFFFFFF) { set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_write_to_mem: a budget of %lld bytes", (long long)d.budget); return nullptr; }
    if (!have_device()) return nullptr;
    const size_t row = (size_t)d.width * (d.color_mode == 0 ? 1u : 3u), px_bytes = row * (size_t)d.height;
    hipStream_t st = thread_stream();
    uint8_t* h = nullptr;
    uint8_t* dev = encode_staging(px_bytes, px_bytes, st, &h);
    if (!dev) { set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_write_to_mem: staging of %zu bytes failed", px_bytes); return nullptr; }
    for (int y = 0; y < d.height; ++y) memcpy(h + row * (size_t)y, static_cast<const uint8_t*>(data) + (ptrdiff_t)pitch * y, row);
    uint8_t* file = static_cast<uint8_t*>(malloc((size_t)d.budget));
    if (!file) { set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_write_to_mem: out of memory"); return nullptr; }
    int rc; int64_t n = 0;
    if (hipMemcpyAsync(dev, h, px_bytes, hipMemcpyHostToDevice, st) != hipSuccess) { (void)hipGetLastError(); rc = set_error(GAMUT_HIP_ERR_HIP, "sqz_write_to_mem: upload failed"); }
    else {
        const uint8_t* src = dev; const int64_t tight = (int64_t)row, zero = 0; int status = 0;
        try { rc = encode_batch(&src, &tight, &d, 1, &zero, file, &n, &status, st); }
        catch (...) { rc = set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_write_to_mem: out of host memory"); }
    }
    (void)hipStreamSynchronize(st);                                 // the pinned buffer the upload reads belongs to the thread's next call
    if (rc != GAMUT_HIP_OK) { free(file); return nullptr; }
    if (void* shrunk = realloc(file, (size_t)n)) file = static_cast<uint8_t*>(shrunk);
    *out_len = (int)n;
    return file;
}

float gamut_hip_sqz_last_encode_stage_ms(int stage) { return stage >= 0 && stage < 3 ? t_stage_ms[stage] : -1.0f; }

} // extern "C"
