// tga_encode.hip -- TGA files on the GPU: the bytes of TGAEncoder (source/gamut/codecs/tga.d:57-281) as saveTGA drives it
// (source/gamut/plugins/tga.d:128-150), many images per call.
//
// The file.  18 header bytes, all zero but byte 2 (10 run-length, 2 raw), width and height (little-endian 16 bit) at 12..15 and
// 24 / 32 bits at 16; byte 17 is 0, so rows go bottom-up; no footer.  l8 and rgb8 give 3 file channels, la8 and rgba8 give 4; a
// pixel is B, G, R (, A).  A row is encoded on its own (:152-280):
//   similar[x] = pixel x equals pixel x - 1 in every file channel, similar[0] = 0;
//   op[x]      = similar[x + 1] ? 0x80 | min(127, ones of `similar` that follow x) : min(127, zeros of `similar` that follow x)
//                (the float comparison at :213-216 reduces to this: one side is always +inf);
//   from x = 0: op[x], then one pixel (0x80 set) or (op & 127) + 1 pixels, and x += (op & 127) + 1.
// op[] is local (128 pixels of look-ahead).  WHICH x the walk visits is the serial chain: a raw packet swallows the first pixel of the
// run behind it unless the cap of 128 ends it just before, and that decides how the run is cut.
//
// The chain as a scan over runs.  Call a maximal stretch of two or more equal pixels a run, P its first pixel, O its last.  A run is
// entered at P + e, e = 1 when the raw packet in front took P.  It is cut into packets of 128 from there; when (O - P + 1 - e) mod
// 128 == 1 its last pixel is left over and starts the raw packets behind it, otherwise they start at O + 1.  Raw packets sit 128
// apart from that entry, and the next run is entered with e = 0 exactly when its first pixel is such a packet start.  So e of a run
// is a function of e of the run in front: one of the four maps of {0, 1}, known at the run's first pixel from P and O of the run in
// front -- both prefix maxima.  The maps compose, so e of every run comes out of a prefix scan; every pixel then knows from P, O and e
// of the run at or in front of it whether it starts a packet, and from op[x] which one.  A wave takes a row 64 pixels at a time: the
// `similar` bits of a group are one ballot, the prefix maxima are count-leading-zeros on masked ballots, the scan of the maps is
// "the last constant map at or below my lane, then the parity of the swaps behind it" on two ballots, and the byte position of a
// pixel is two population counts.  What crosses a group is P, O, e and the byte count: no barrier, no LDS, nothing that waits.
// (Chosen over pointer doubling on next(x), tga.hip's way: that takes log2(window) rounds over a jump table in LDS; this takes a
// fixed handful of wave-wide operations per 64 pixels and keeps the row in registers.)
//
// Three launches on the call's stream, whatever the batch holds:
//   k_tgaenc_rows     a wave per row of the batch: the row's byte length into scratch;
//   k_tgaenc_offsets  a workgroup per file: prefix sums of the row lengths in file order (bottom row first) behind the 18 header
//                     bytes, and the file's length;
//   k_tgaenc_write    a wave per row again: the packets are recomputed (reading the source twice costs less traffic than writing and
//                     gathering bound-sized scratch slots), assembled kWin pixels at a time in the wave's LDS and stored as aligned
//                     16-byte chunks with byte head and tail (flush_run); the wave of a file's first row writes the header.
// Nothing outside [out_offset, out_offset + out_len) is written.  Raw files (rle 0) take the same path with no packet bytes.
//
// DELIBERATE DEVIATIONS: the reference refuses only a dimension above 65535 and the other pixel types; here width or height 0 (it
// writes a header and nothing) and a bound 18 + w * h * (file channels + 1) above 2^31 - 1 are refused too.
#include "encode_host.hpp"
#include "device_util.hpp"

namespace gamut {
namespace {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kRowsPerBlock = kThreads / kWave;                              // a wave per row
constexpr int kWin = 512;                                                    // pixels assembled in LDS between two flushes
constexpr int kWinGroups = kWin / kWave;
constexpr int kStageDwords = kWin * 5 / 4 + 8;                               // kWin packets of one pixel, spare dwords for flush_run
constexpr int kHeader = 18;

struct EncImg {
    const uint8_t* src; int64_t pitch; int64_t out_off;
    uint32_t w, h;
    uint32_t row0;                                                           // rows [row0, row0 + h) of the batch, in file order
    uint8_t  comp, fc, rle, pad;                                             // source channels, file channels
};

__device__ __forceinline__ void wave_sync()                                  // compiler order only: a wave's LDS accesses are served in issue order
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int top_bit(uint64_t m) { return 63 - __builtin_clzll(m); }     // m != 0

// bits of three consecutive groups' masks from position lane + 1 of the first: how many ones in a row, capped at 127; *first = bit 0
__device__ __forceinline__ uint32_t ones_behind(uint64_t m0, uint64_t m1, uint64_t m2, uint32_t lane, uint32_t* first)
{
    const uint32_t sh = lane + 1;                                            // 1..64
    const uint64_t lo = sh == 64 ? m1 : (m0 >> sh) | (m1 << (64 - sh));
    const uint64_t hi = sh == 64 ? m2 : (m1 >> sh) | (m2 << (64 - sh));
    *first = (uint32_t)(lo & 1u);
    const uint32_t n = ~lo ? (uint32_t)__builtin_ctzll(~lo) : 64u + (~hi ? (uint32_t)__builtin_ctzll(~hi) : 64u);
    return min(n, 127u);
}

// the file's pixel x as B | G << 8 | R << 16 | A << 24 (A = 255 without an alpha channel): scanline_convert_* and the swap :157-179
__device__ __forceinline__ uint32_t load_px(const uint8_t* row, uint32_t x, uint32_t comp, bool dwords)
{
    const uint8_t* p = row + (size_t)x * comp;
    if (comp == 1) return p[0] * 0x010101u | 0xFF000000u;
    if (comp == 2) return p[0] * 0x010101u | (uint32_t)p[1] << 24;
    if (comp == 3) return p[2] | (uint32_t)p[1] << 8 | (uint32_t)p[0] << 16 | 0xFF000000u;
    const uint32_t raw = dwords ? *reinterpret_cast<const uint32_t*>(p) : p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
    return __builtin_amdgcn_perm(raw, raw, 0x03000102u);                     // R G B A -> B G R A
}

// where the raw packets behind the run [p, o] start when the run was entered at p + e; 0 in front of the row's first run
__device__ __forceinline__ int32_t raw_entry(int32_t p, int32_t o, uint32_t e)
{
    if (p < 0) return 0;
    return (((uint32_t)(o - p + 1) - e) & 127u) == 1u ? o : o + 1;
}

// File row j of an image by one wave; every lane of the wave is here.  kWrite: the bytes go to dst through the wave's LDS S.
// Returns the row's byte length.
template <bool kWrite>
__device__ __forceinline__ uint32_t encode_row(const EncImg& im, uint32_t j, uint8_t* dst, uint32_t* S, uint32_t lane)
{
    const uint32_t w = im.w, C = im.fc, groups = (w + kWave - 1) / kWave;
    const uint8_t* row = im.src + (int64_t)(im.h - 1 - j) * im.pitch;        // rows bottom-up (plugins/tga.d:140)
    const bool dwords = im.comp == 4 && ((uintptr_t)row & 3u) == 0;
    const bool rle = im.rle != 0;
    const uint64_t le = ~0ull >> (63 - lane), lt = le >> 1;                  // lanes <= mine, lanes < mine
    uint32_t lastv = 0;
    // group g: its pixels, M = similar, Z = valid and not similar
    auto fetch = [&](uint32_t g, uint32_t& v, uint64_t& M, uint64_t& Z) {
        const uint32_t x = g * kWave + lane;
        const bool valid = g < groups && x < w;
        v = valid ? load_px(row, x, im.comp, dwords) : 0u;
        uint32_t prev = __shfl_up(v, 1, kWave);
        if (lane == 0) prev = lastv;
        M = rle ? __ballot(valid && x > 0 && v == prev) : 0ull;
        Z = __ballot(valid) & ~M;
        lastv = __shfl(v, kWave - 1, kWave);
    };
    uint32_t v0, v1, v2; uint64_t M0, M1, M2, Z0, Z1, Z2;                    // groups g, g + 1, g + 2: op[] looks 128 pixels ahead
    fetch(0, v0, M0, Z0); fetch(1, v1, M1, Z1); fetch(2, v2, M2, Z2);
    int32_t Pc = -1, Oc = -1;                                                // first and last pixel of the last run in front of the group
    uint32_t e_in = 0;                                                       // how that run was entered
    uint32_t row_bytes = 0, fill = 0;                                        // flushed, and waiting in S
    for (uint32_t g = 0; g < groups; ++g) {
        const uint32_t x = g * kWave + lane;
        const bool valid = x < w;
        bool start = false, emit = valid;
        uint32_t op = 0;
        if (rle) {                                                           // (uniform over the wave)
            uint32_t next_similar, unused;
            const uint32_t n_same = ones_behind(M0, M1, M2, lane, &next_similar), n_diff = ones_behind(Z0, Z1, Z2, lane, &unused);
            op = next_similar ? 0x80u | n_same : n_diff;                     // :213-227
            const uint64_t first = ~M0 & (M0 >> 1 | M1 << 63);               // first pixels of runs
            const bool similar = (M0 >> lane) & 1u, is_first = (first >> lane) & 1u;
            const uint64_t tp = first & le, to = M0 & le, tpx = first & lt;
            const int32_t P = tp ? (int32_t)(g * kWave) + top_bit(tp) : Pc, O = to ? (int32_t)(g * kWave) + top_bit(to) : Oc;
            const int32_t Px = tpx ? (int32_t)(g * kWave) + top_bit(tpx) : Pc;             // the run in front of a first pixel (its O is O)
            // the map e -> e at a run's first pixel, the identity elsewhere
            bool f0 = false, f1 = true;
            if (is_first) { f0 = ((x - (uint32_t)raw_entry(Px, O, 0u)) & 127u) != 0; f1 = ((x - (uint32_t)raw_entry(Px, O, 1u)) & 127u) != 0; }
            const uint64_t F0 = __ballot(f0), F1 = __ballot(f1), constant = ~(F0 ^ F1), swap = F0 & ~F1;
            auto state = [&](uint64_t upto) -> uint32_t {                    // e behind the lanes of `upto` (lanes 0 .. some lane)
                const uint64_t c = constant & upto;
                uint32_t base = e_in; uint64_t span = upto;
                if (c) { const int k = top_bit(c); base = (uint32_t)(F0 >> k) & 1u; span = upto & ~(((uint64_t)2 << k) - 1); }
                return base ^ ((uint32_t)__builtin_popcountll(swap & span) & 1u);
            };
            const uint32_t e = state(le);
            if (valid) {
                if (similar || is_first) {                                   // inside the run that starts at P
                    const uint32_t k = x - (uint32_t)P;
                    if (k < e) { start = false; emit = true; }               // taken by the raw packet in front
                    else { start = ((k - e) & 127u) == 0; emit = start; }    // a packet start (op says which), or inside a run-length packet
                } else {
                    start = ((x - (uint32_t)raw_entry(P, O, e)) & 127u) == 0;
                }
            }
            if (first) Pc = (int32_t)(g * kWave) + top_bit(first);
            if (M0) Oc = (int32_t)(g * kWave) + top_bit(M0);
            e_in = state(~0ull);
        }
        const uint64_t sm = __ballot(start), em = __ballot(emit);
        if (kWrite) {
            uint8_t* Sb = reinterpret_cast<uint8_t*>(S);
            uint32_t off = fill + (uint32_t)__builtin_popcountll(sm & lt) + C * (uint32_t)__builtin_popcountll(em & lt);
            if (start) Sb[off++] = (uint8_t)op;
            if (emit) {
                Sb[off] = (uint8_t)v0; Sb[off + 1] = (uint8_t)(v0 >> 8); Sb[off + 2] = (uint8_t)(v0 >> 16);
                if (C == 4) Sb[off + 3] = (uint8_t)(v0 >> 24);
            }
        }
        fill += (uint32_t)__builtin_popcountll(sm) + C * (uint32_t)__builtin_popcountll(em);
        v0 = v1; M0 = M1; Z0 = Z1; v1 = v2; M1 = M2; Z1 = Z2;
        fetch(g + 3, v2, M2, Z2);
        if ((g + 1) % kWinGroups == 0 || g + 1 == groups) {
            if (kWrite) { wave_sync(); flush_run<kWave>(S, dst + row_bytes, fill, lane); wave_sync(); }
            row_bytes += fill; fill = 0;
        }
    }
    return row_bytes;
}

__global__ __launch_bounds__(kThreads) void k_tgaenc_rows(const EncImg* imgs, int n_img, uint32_t n_rows, uint32_t* row_len)
{
    const uint32_t u = blockIdx.x * kRowsPerBlock + threadIdx.x / kWave, lane = threadIdx.x % kWave;
    if (u >= n_rows) return;                                                 // (uniform over the wave)
    const EncImg im = imgs[find_unit<&EncImg::row0>(imgs, n_img, u)];
    const uint32_t n = im.rle ? encode_row<false>(im, u - im.row0, nullptr, nullptr, lane) : im.w * im.fc;
    if (lane == 0) row_len[u] = n;
}

// row lengths -> the rows' positions in their file, in place; one workgroup per file, rows in file order
__global__ __launch_bounds__(kThreads) void k_tgaenc_offsets(const EncImg* imgs, uint32_t* rows, uint32_t* file_len)
{
    __shared__ uint32_t wave_sum[kRowsPerBlock];
    const EncImg im = imgs[blockIdx.x];
    const uint32_t tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    uint32_t running = kHeader;
    for (uint32_t j0 = 0; j0 < im.h; j0 += kThreads) {                       // (uniform over the workgroup; at most 256 turns)
        const uint32_t j = j0 + tid, len = j < im.h ? rows[im.row0 + j] : 0u;
        uint32_t incl = len;
        for (int d = 1; d < kWave; d <<= 1) { const uint32_t t = __shfl_up(incl, d, kWave); if (lane >= (uint32_t)d) incl += t; }
        if (lane == kWave - 1) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t k = 0; k < (uint32_t)kRowsPerBlock; ++k) { if (k < wave) before += wave_sum[k]; total += wave_sum[k]; }
        if (j < im.h) rows[im.row0 + j] = running + before + incl - len;
        running += total;
        __syncthreads();
    }
    if (tid == 0) file_len[blockIdx.x] = running;
}

__global__ __launch_bounds__(kThreads) void k_tgaenc_write(const EncImg* imgs, int n_img, uint32_t n_rows, const uint32_t* row_off, uint8_t* out)
{
    __shared__ uint32_t stage[kRowsPerBlock][kStageDwords];
    const uint32_t wave = threadIdx.x / kWave, u = blockIdx.x * kRowsPerBlock + wave, lane = threadIdx.x % kWave;
    if (u >= n_rows) return;                                                 // (uniform over the wave; the kernel has no barrier)
    const EncImg im = imgs[find_unit<&EncImg::row0>(imgs, n_img, u)];
    const uint32_t j = u - im.row0;
    uint8_t* file = out + im.out_off;
    if (j == 0 && lane < (uint32_t)kHeader) {                                // :121-133
        const uint32_t b = lane == 2 ? (im.rle ? 10u : 2u) : lane == 12 ? im.w & 255u : lane == 13 ? im.w >> 8 : lane == 14 ? im.h & 255u :
                           lane == 15 ? im.h >> 8 : lane == 16 ? im.fc * 8u : 0u;
        file[lane] = (uint8_t)b;
    }
    encode_row<true>(im, j, file + row_off[u], stage[wave], lane);
}

int file_channels(int comp) { return comp == 1 || comp == 3 ? 3 : 4; }       // :92-113

int64_t encode_bound(int w, int h, int comp)
{
    if (comp < 1 || comp > 4 || w < 1 || h < 1 || w > 65535 || h > 65535) return 0;
    const int64_t b = kHeader + (int64_t)w * h * (file_channels(comp) + 1);
    return b > 0x7fffffffLL ? 0 : b;
}

// Measurements (tools/tga_encode_bench.py): with GAMUT_HIP_TGA_TIMING=1 the encode call brackets its three launches with events and
// keeps the GPU times of the calling thread's last call.
thread_local float t_last_encode_stage_ms[3] = { -1.0f, -1.0f, -1.0f };

int encode_batch(const uint8_t* const* src, const int64_t* src_pitch, const int32_t* width, const int32_t* height, const int32_t* comp,
                 const int32_t* rle, int count, const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host, hipStream_t stream)
{
    std::vector<EncImg> imgs; std::vector<int> which;
    int first_bad = -1;
    uint64_t rows = 0;
    for (int i = 0; i < count; ++i) {
        out_len[i] = 0;
        const bool ok = encode_bound(width[i], height[i], comp[i]) > 0 && src[i] && out_offset[i] >= 0;
        if (status_host) status_host[i] = ok ? GAMUT_HIP_OK : GAMUT_HIP_ERR_INVALID_ARG;
        if (!ok) { if (first_bad < 0) first_bad = i; continue; }
        EncImg im{};
        im.src = src[i]; im.pitch = src_pitch[i]; im.out_off = out_offset[i];
        im.w = (uint32_t)width[i]; im.h = (uint32_t)height[i];
        im.comp = (uint8_t)comp[i]; im.fc = (uint8_t)file_channels(comp[i]); im.rle = (uint8_t)(!rle || rle[i] != 0);
        im.row0 = (uint32_t)rows;
        rows += im.h;
        if (rows > 0x7FFFFFFFull) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "tga_encode: batch of more than 2^31 rows");
        imgs.push_back(im); which.push_back(i);
    }
    if (!imgs.empty()) {
        const int n = (int)imgs.size();
        const size_t o_img = 0, o_len = up256(n * sizeof(EncImg)), o_rows = o_len + up256((size_t)n * 4), total = o_rows + up256((size_t)rows * 4);
        static thread_local PerDevice<DeviceScratch> scratch_pd;
        static thread_local PerDevice<PinnedScratch> pinned_pd;
        uint8_t* d = (uint8_t*)scratch_pd.cur().get(total, stream);
        uint8_t* h = pinned_pd.cur().get(o_rows, stream);
        if (!d || !h) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "tga_encode: scratch allocation of %zu bytes failed", total);
        memcpy(h + o_img, imgs.data(), n * sizeof(EncImg));
        GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, n * sizeof(EncImg), hipMemcpyHostToDevice, stream));
        const EncImg* dimg = (const EncImg*)(d + o_img);
        uint32_t* drows = (uint32_t*)(d + o_rows);
        const uint32_t n_rows = (uint32_t)rows, blocks = (n_rows + kRowsPerBlock - 1) / kRowsPerBlock;
        static const bool timing = env_flag("GAMUT_HIP_TGA_TIMING");
        KernelTimer<4> timer(timing);
        timer.mark(stream);
        hipLaunchKernelGGL(k_tgaenc_rows, dim3(blocks), dim3(kThreads), 0, stream, dimg, n, n_rows, drows);
        timer.mark(stream);
        hipLaunchKernelGGL(k_tgaenc_offsets, dim3((uint32_t)n), dim3(kThreads), 0, stream, dimg, drows, (uint32_t*)(d + o_len));
        timer.mark(stream);
        hipLaunchKernelGGL(k_tgaenc_write, dim3(blocks), dim3(kThreads), 0, stream, dimg, n, n_rows, (const uint32_t*)drows, out);
        if (int rc = launch_status("tga_encode")) return rc;
        timer.mark(stream);
        GAMUT_HIP_CHECK(hipMemcpyAsync(h + o_len, d + o_len, (size_t)n * 4, hipMemcpyDeviceToHost, stream));
        GAMUT_HIP_CHECK(hipStreamSynchronize(stream));
        timer.finish(t_last_encode_stage_ms);
        const uint32_t* lens = (const uint32_t*)(h + o_len);
        for (int k = 0; k < n; ++k) out_len[which[(size_t)k]] = lens[k];
    }
    if (first_bad >= 0) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "image %d: tga_encode: refused shape or source", first_bad);
    return GAMUT_HIP_OK;
}

} // namespace
} // namespace gamut

using namespace gamut;

extern "C" {

int64_t gamut_hip_tga_encode_bound(int width, int height, int comp) { return encode_bound(width, height, comp); }

int gamut_hip_tga_encode_window(void) { return kWin; }

int gamut_hip_tga_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const int32_t* width, const int32_t* height,
                                      const int32_t* comp, const int32_t* rle, int count, const int64_t* out_offset, uint8_t* out,
                                      int64_t* out_len, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!src || !src_pitch || !width || !height || !comp || !out_offset || !out || !out_len)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "tga_encode_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return encode_batch(src, src_pitch, width, height, comp, rle, count, out_offset, out, out_len, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "tga_encode_batch_device: out of host memory");
    }
}

void* gamut_hip_tga_write_to_mem(const void* data, int pitch, int w, int h, int comp, int rle, int* out_len)
{
    clear_error();
    if (!data || !out_len || encode_bound(w, h, comp) == 0) {
        set_error(GAMUT_HIP_ERR_INVALID_ARG, "tga_write_to_mem: invalid arguments"); return nullptr;
    }
    if (!have_device()) return nullptr;
    const int32_t W = w, H = h, Cc = comp, R = rle;
    return encode_host_image("tga_write_to_mem", HostRows{ data, pitch, (size_t)w * comp, h, 1, 0 }, (size_t)encode_bound(w, h, comp), out_len,
        [&](const uint8_t* src, int64_t spitch, int64_t, int64_t off, uint8_t* d, int64_t* n, hipStream_t st) {
            int status = 0;
            return encode_batch(&src, &spitch, &W, &H, &Cc, &R, 1, &off, d, n, &status, st);
        });
}

float gamut_hip_tga_last_encode_kernel_ms(void)
{
    const float* t = t_last_encode_stage_ms;
    return t[0] < 0 || t[1] < 0 || t[2] < 0 ? -1.0f : t[0] + t[1] + t[2];
}

float gamut_hip_tga_last_encode_stage_ms(int stage) { return stage >= 0 && stage < 3 ? t_last_encode_stage_ms[stage] : -1.0f; }

} // extern "C"
