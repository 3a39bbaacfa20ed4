// dds_encode.hip -- DDS files that hold BC7 on the GPU: the bytes of saveDDS (source/gamut/plugins/dds.d:47-216), which packs every
// 4 x 4 tile with bc7enc16_compress_block (source/gamut/codecs/bc7enc16.d:1825-1857) on the parameters of
// bc7enc16_compress_block_params_init: 64 mode-1 partitions, least squares, the partition filterbank, uber level 0, perceptual weights.
//
// The file.  "DDS ", DDSURFACEDESC2 (124 bytes), DDS_HEADER_DXT10 (20 bytes): 148 bytes, zero but for the fields header_dword() names;
// then ((w + 3) / 4) * ((h + 3) / 4) blocks of 16 bytes in row-major order.  A tile is gathered as l8 -> (v, v, v, 255), la8 ->
// (v, v, v, a), rgb8 -> (r, g, b, 255), rgba8 as it is; a position outside the image is (0, 0, 0, 0), so an edge tile of an image whose
// size is no multiple of 4 holds alpha 0 and takes the alpha path.
//
// A tile.  Mode 6 (one subset, 7-bit endpoints with a p-bit each, 4-bit selectors) always; an opaque tile whose mode-6 error is above
// 0 also tries mode 1 (two subsets of the partition estimate_partition picks, 6-bit rgb endpoints with a shared p-bit, 3-bit
// selectors) and takes it on a strictly smaller error.  A subset is fitted by color_cell_compression: mean and principal axis in
// float, the projections' extremes as endpoints, find_optimal_solution (quantise per p-bit, fixDegenerateEndpoints, evaluate_solution:
// every pixel against every interpolated colour, YCbCr distance, summed in 64 bits), one least-squares refit from the selectors, and
// for mode 1 the subset as its mean colour through the 256 x 2 table of best endpoints for one value (:1304-1318; that step stands
// behind the uber-level block, not in it).  It returns 0 as soon as a fit reports error 0.
//
// The kernel.  One launch per call: 16 lanes per tile, four tiles per wave, one lane per pixel; a flat tile index is mapped to
// (image, tile) through the records' tile0, so a workgroup serves tiles of any image and 600 tiny images cost what their tiles cost.
//   * the integer work is per lane: evaluate_solution's search for a lane's own pixel, the sums by butterflies over the 16 lanes
//     (exact in any order); estimate_partition gives every lane four of the 64 partitions to estimate in full, then applies the
//     reference's sequential selection (first 14, key partition, predictors for 14..34, checkerboard stop, stop at 0) to the 64 sums.
//     The early exits inside color_cell_compression_est never change a selection: a cut sum is already above the best.
//   * the float sections are uniform over a tile's 16 lanes: every lane runs them redundantly in the reference's order, pixel i
//     fetched by a cross-lane read, "the pixels of a subset in index order" as a walk over the bits of the subset's mask.  IEEE
//     binary32, every operation rounded on its own (-ffp-contract=off), correctly rounded division and square root, denormals kept;
//     no sum is turned into a tree.
//   * every float -> int conversion goes through f2i(), which gives what cvttss2si gives (INT_MIN for NaN and for what does not fit):
//     a NaN from a degenerate least-squares system passes saturate().
//   * no per-thread array is indexed at run time (no scratch): interpolated colours are recomputed from the weight, subsets are masks.
//   * the 16 bytes of a block leave as four dwords where the address allows, else as 16 bytes from 16 lanes; the lanes of an image's
//     tile 0 write its header.  Nothing outside [out_offset, out_offset + 148 + 16 * tiles) is written.
// The selector-weight tables (the reference's 6-decimal literals) and the 256 x 2 table are computed on the host and copied to
// each device once.
//
// DELIBERATE DEVIATION: the reference's `int numBlocks` wraps for huge images; a file above 2^31 - 1 bytes is refused here.
#include "encode_host.hpp"
#include "device_util.hpp"
#include <climits>
#include <cmath>
#include <mutex>

namespace gamut {
namespace {

constexpr int kThreads = 256;
constexpr int kLanes = 16;                                                   // per tile
constexpr int kTilesPerBlock = kThreads / kLanes;
constexpr int kHeader = 148;

struct EncImg {
    const uint8_t* src; int64_t pitch; int64_t out_off;
    uint32_t w, h, bw;
    uint32_t tile0;                                                          // tiles [tile0, tile0 + bw * bh) of the batch
    uint32_t comp;
};

struct Tables {
    uint32_t opt1[256][2];                                                   // g_bc7_mode_1_optimal_endpoints: error | lo << 16 | hi << 24
    float wx3[8][4], wx4[16][4];                                             // g_bc7_weights3x / 4x
};
__device__ Tables g_tab;

__device__ const uint32_t kW3[8] = { 0, 9, 18, 27, 37, 46, 55, 64 };
__device__ const uint32_t kW4[16] = { 0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64 };
// bit i of entry p: the subset of pixel i in 2-subset partition p; the second subset's anchor pixel
__device__ const uint16_t kPart2[64] = {
    0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80, 0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8, 0xFF00, 0xFFF0, 0xF000,
    0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE, 0x088C, 0x3110, 0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C,
    0xAAAA, 0xF0F0, 0x5A5A, 0x33CC, 0x3C3C, 0x55AA, 0x9696, 0xA55A, 0x73CE, 0x13C8, 0x324C, 0x3BDC, 0x6996, 0xC33C, 0x9966, 0x0660,
    0x0272, 0x04E4, 0x4E40, 0x2720, 0xC936, 0x936C, 0x39C6, 0x639C, 0x9336, 0x9CC6, 0x817E, 0xE718, 0xCCF0, 0x0FCC, 0x7744, 0xEE22 };
__device__ const uint8_t kAnchor2[64] = {
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
    15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6, 6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15 };
// estimate_partition: s_sorted_partition_order, and g_partition_predictors (which key partitions admit a pattern of slots 14..34)
__device__ const uint8_t kOrder[64] = {
    0, 13, 1, 2, 15, 14, 10, 16, 3, 23, 26, 6, 7, 21, 19, 29, 8, 4, 9, 20, 5, 31, 22, 17, 18, 11, 12, 30, 24, 25, 28, 27,
    32, 33, 34, 45, 46, 51, 49, 50, 48, 38, 39, 37, 53, 52, 54, 36, 57, 58, 55, 41, 40, 42, 43, 59, 44, 56, 47, 35, 60, 63, 62, 61 };
constexpr uint32_t bits_of(std::initializer_list<int> l) { uint32_t m = 0; for (int b : l) m |= 1u << b; return m; }
__device__ const uint32_t kPredict[35] = {
    ~0u, ~0u, ~0u, ~0u, ~0u, bits_of({ 1, 2, 8 }), bits_of({ 1, 3, 7 }), ~0u, ~0u, bits_of({ 2, 8, 16 }), bits_of({ 7, 3, 15 }), ~0u,
    bits_of({ 8, 14, 16 }), bits_of({ 7, 14, 15 }), ~0u, ~0u, ~0u, ~0u, bits_of({ 14, 15 }), bits_of({ 16, 22, 14 }), bits_of({ 17, 24, 14 }),
    bits_of({ 2, 14, 15, 1 }), ~0u, bits_of({ 1, 3, 14, 16, 22 }), ~0u, bits_of({ 1, 2, 15, 17, 24 }), bits_of({ 1, 3, 22 }), ~0u, ~0u, ~0u,
    bits_of({ 14, 15, 16, 17 }), ~0u, ~0u, bits_of({ 1, 2, 3, 27, 4, 24 }), bits_of({ 14, 15, 16, 11, 17, 27 }) };
// bc7enc16_compress_block :1837-1842 on the weights (128, 64, 16, 32): 512, (int)(256 * 0.40322...), (int)(64 * 0.29042...), 128
constexpr uint32_t kWeightL = 512, kWeightCr = 103, kWeightCb = 18, kWeightA = 128;

// ---- cross-lane: a tile's 16 lanes are always in the same control flow, and read only one another
__device__ __forceinline__ uint32_t bcast(uint32_t v, uint32_t i) { return (uint32_t)__shfl((int)v, (int)i, kLanes); }
__device__ __forceinline__ uint64_t bcast64(uint64_t v, uint32_t i)
{
    return (uint64_t)bcast((uint32_t)v, i) | (uint64_t)bcast((uint32_t)(v >> 32), i) << 32;
}
__device__ __forceinline__ uint64_t sum16(uint64_t v)
{
    for (int d = 1; d < kLanes; d <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, kLanes), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, kLanes);
        v += (uint64_t)lo | (uint64_t)hi << 32;
    }
    return v;
}
__device__ __forceinline__ uint64_t or16(uint64_t v)
{
    for (int d = 1; d < kLanes; d <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, kLanes), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, kLanes);
        v |= (uint64_t)lo | (uint64_t)hi << 32;
    }
    return v;
}
__device__ __forceinline__ uint32_t tile_ballot(bool p) { return (uint32_t)(__ballot(p) >> (threadIdx.x & 48u)) & 0xFFFFu; }

// cast(int) of a float as the reference's x86-64 build does it (cvttss2si): INT_MIN for NaN and for what does not fit
__device__ __forceinline__ int f2i(float f) { return f >= -2147483648.0f && f < 2147483648.0f ? (int)f : INT_MIN; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
__device__ __forceinline__ float saturate(float v) { if (v < 0.0f) v = 0.0f; else if (v > 1.0f) v = 1.0f; return v; }      // a NaN passes
__device__ __forceinline__ uint32_t ch(uint32_t px, int c) { return (px >> (8 * c)) & 255u; }

struct Ycc { int l, cr, cb; };
__device__ __forceinline__ Ycc ycc(uint32_t r, uint32_t g, uint32_t b)
{
    Ycc y; y.l = (int)(r * 109u + g * 366u + b * 37u); y.cr = (int)(r << 9) - y.l; y.cb = (int)(b << 9) - y.l; return y;
}
// compute_color_distance_rgb, perceptual
__device__ __forceinline__ uint32_t dist_ycc(const Ycc& a, const Ycc& b)
{
    const int dl = (a.l - b.l) >> 8, dcr = (a.cr - b.cr) >> 8, dcb = (a.cb - b.cb) >> 8;
    return kWeightL * (uint32_t)(dl * dl) + kWeightCr * (uint32_t)(dcr * dcr) + kWeightCb * (uint32_t)(dcb * dcb);
}

struct Cell {                                                                // color_cell_compressor_params; uniform over the tile
    uint32_t mode, mask, n;                                                  // mask: the subset's pixels
    uint32_t nw, comp_bits;
    bool has_alpha, share_pbit;
};
struct Res {                                                                 // color_cell_compressor_results; sel is the lane's own
    uint64_t best; uint32_t lo, hi, pb0, pb1, sel;
};

// scale_color on four packed components of comp_bits + 1 bits
__device__ __forceinline__ uint32_t scale_color(uint32_t c, const Cell& p)
{
    return p.comp_bits == 7 ? c : ((c << 1) & 0xFEFEFEFEu) | ((c >> 6) & 0x01010101u);
}
__device__ __forceinline__ uint32_t lerp64(uint32_t a, uint32_t b, uint32_t w) { return ((a * (64u - w) + b * w + 32u) >> 6) & 255u; }

// the error of the lane's pixel (0 outside the subset) summed over the tile
__device__ __forceinline__ uint64_t pack_one_color(const Cell& p, Res& r, uint32_t cr, uint32_t cg, uint32_t cb, const Ycc& mine, bool member)
{
    uint32_t best_err = ~0u, best_p = 0;
    for (uint32_t pb = 0; pb < 2; ++pb) {
        const uint32_t e = (g_tab.opt1[cr][pb] & 0xFFFFu) + (g_tab.opt1[cg][pb] & 0xFFFFu) + (g_tab.opt1[cb][pb] & 0xFFFFu);
        if (e < best_err) { best_err = e; best_p = pb; }
    }
    const uint32_t er = g_tab.opt1[cr][best_p], eg = g_tab.opt1[cg][best_p], eb = g_tab.opt1[cb][best_p];
    r.lo = ((er >> 16) & 255u) | ((eg >> 16) & 255u) << 8 | ((eb >> 16) & 255u) << 16;
    r.hi = (er >> 24) | (eg >> 24) << 8 | (eb >> 24) << 16;
    r.pb0 = best_p; r.pb1 = 0;
    uint32_t q[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        uint32_t low = ((ch(r.lo, i) << 1) | best_p) << 1, high = ((ch(r.hi, i) << 1) | best_p) << 1;
        low |= low >> 7; high |= high >> 7;
        q[i] = lerp64(low, high, 18u);
    }
    const uint64_t total = sum16(member ? dist_ycc(ycc(q[0], q[1], q[2]), mine) : 0u);
    r.best = total;
    return total;
}

__device__ __forceinline__ void evaluate_solution(uint32_t lo, uint32_t hi, uint32_t pb0, uint32_t pb1, const Cell& p, Res& r, uint32_t px,
                                                  const Ycc& mine, bool member)
{
    const uint32_t pmin = pb0, pmax = p.share_pbit ? pb0 : pb1;
    const uint32_t amin = scale_color(((lo << 1) & 0xFEFEFEFEu) | pmin * 0x01010101u, p), amax = scale_color(((hi << 1) & 0xFEFEFEFEu) | pmax * 0x01010101u, p);
    const uint32_t* W = p.nw == 16 ? kW4 : kW3;
    const int my_a = (int)ch(px, 3);
    uint32_t best = ~0u, best_sel = 0;
    for (uint32_t j = 0; j < p.nw; ++j) {                                     // weight 0 gives amin and weight 64 amax exactly
        const uint32_t w = W[j];
        uint32_t e = dist_ycc(ycc(lerp64(ch(amin, 0), ch(amax, 0), w), lerp64(ch(amin, 1), ch(amax, 1), w), lerp64(ch(amin, 2), ch(amax, 2), w)), mine);
        if (p.has_alpha) { const int da = (int)lerp64(ch(amin, 3), ch(amax, 3), w) - my_a; e += kWeightA * (uint32_t)(da * da); }
        if (e < best) { best = e; best_sel = j; }
    }
    const uint64_t total = sum16(member ? best : 0u);
    if (total < r.best) { r.best = total; r.lo = lo; r.hi = hi; r.pb0 = pb0; r.pb1 = pb1; r.sel = best_sel; }
}

// one endpoint component for p-bit pb; the reference multiplies and adds in int, which wraps
__device__ __forceinline__ uint32_t quant_pbit(float x, float scalep, int pb, int iscalep)
{
    const float a = x * scalep, b = a - (float)pb, c = b / 2.0f, d = c + .5f;
    const int v = (int)((uint32_t)f2i(d) * 2u + (uint32_t)pb);
    return (uint32_t)clampi(v, pb, iscalep - 1 + pb);
}

__device__ __forceinline__ uint64_t find_optimal_solution(const Cell& p, const float* xl_in, const float* xh_in, Res& r, uint32_t px, const Ycc& mine,
                                                          bool member)
{
    float xl[4], xh[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) { xl[c] = saturate(xl_in[c]); xh[c] = saturate(xh_in[c]); }
    const int iscalep = (1 << (p.comp_bits + 1)) - 1, comps = p.has_alpha ? 4 : 3;
    const float scalep = (float)iscalep;
    uint32_t bp0 = 0, bp1 = 0, bmin = 0, bmax = 0;
    float best0 = 1e+9f, best1 = 1e+9f;                                      // (1e+9 is a float)
#pragma unroll
    for (int pb = 0; pb < 2; ++pb) {
        uint32_t xmin = 0, xmax = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) { xmin |= quant_pbit(xl[c], scalep, pb, iscalep) << (8 * c); xmax |= quant_pbit(xh[c], scalep, pb, iscalep) << (8 * c); }
        const uint32_t slo = scale_color(xmin, p), shi = scale_color(xmax, p);
        if (!p.share_pbit) {
            float e0 = 0, e1 = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < comps) {
                const float a = xl[i] * 255.0f, da = (float)ch(slo, i) - a, b = xh[i] * 255.0f, db = (float)ch(shi, i) - b;
                e0 += da * da; e1 += db * db;
            }
            if (e0 < best0) { best0 = e0; bp0 = (uint32_t)pb; bmin = (xmin >> 1) & 0x7F7F7F7Fu; }
            if (e1 < best1) { best1 = e1; bp1 = (uint32_t)pb; bmax = (xmax >> 1) & 0x7F7F7F7Fu; }
        } else {
            float e = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < comps) {
                const float a = (float)ch(slo, i) / 255.0f, da = a - xl[i], b = (float)ch(shi, i) / 255.0f, db = b - xh[i];
                const float s = da * da + db * db;
                e += s;
            }
            if (e < best0) { best0 = e; bp0 = bp1 = (uint32_t)pb; bmin = (xmin >> 1) & 0x7F7F7F7Fu; bmax = (xmax >> 1) & 0x7F7F7F7Fu; }
        }
    }
    if (p.mode == 1) {                                                       // fixDegenerateEndpoints, iscale = iscalep >> 1
        const uint32_t iscale = (uint32_t)iscalep >> 1;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t mn = ch(bmin, i), mx = ch(bmax, i), one = 1u << (8 * i);
            if (mn != mx || !(fabsf(xl[i] - xh[i]) > 0.0f)) continue;
            if (mn > (iscale >> 1)) { if (mn > 0) bmin -= one; else if (mx < iscale) bmax += one; }
            else { if (mx < iscale) bmax += one; else if (mn > 0) bmin -= one; }
        }
    }
    if (r.best == ~0ull || bmin != r.lo || bmax != r.hi || bp0 != r.pb0 || bp1 != r.pb1) evaluate_solution(bmin, bmax, bp0, bp1, p, r, px, mine, member);
    return r.best;
}

__device__ __forceinline__ void normalize4(float* v)
{
    float s = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    if (s != 0.0f) { s = 1.0f / sqrtf(s); v[0] *= s; v[1] *= s; v[2] *= s; v[3] *= s; }
}
__device__ __forceinline__ float dot4(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }

// color_cell_compression at uber level 0 with least squares; every lane of the tile is here
__device__ __forceinline__ uint64_t color_cell_compression(const Cell& p, Res& r, uint32_t px, const Ycc& mine, bool member)
{
    r.best = ~0ull; r.lo = r.hi = r.pb0 = r.pb1 = r.sel = 0;
    const uint32_t first = (uint32_t)__builtin_ctz(p.mask);
    if (p.mode == 1) {
        const uint32_t c0 = bcast(px, first);
        if ((tile_ballot(member && ((px ^ c0) & 0xFFFFFFu) != 0)) == 0) {    // the subset is one colour
            r.sel = 2;
            return pack_one_color(p, r, ch(c0, 0), ch(c0, 1), ch(c0, 2), mine, member);
        }
    }
    float mean[4] = { 0, 0, 0, 0 }, mean_scaled[4], axis[4];
    for (uint32_t i = first; i < 16; ++i) {
        if (!((p.mask >> i) & 1u)) continue;
        const uint32_t c = bcast(px, i);
#pragma unroll
        for (int k = 0; k < 4; ++k) mean[k] = mean[k] + (float)ch(c, k);
    }
    const float inv_n = 1.0f / (float)p.n, inv_n255 = 1.0f / ((float)p.n * 255.0f);
#pragma unroll
    for (int k = 0; k < 4; ++k) { mean_scaled[k] = mean[k] * inv_n; mean[k] = saturate(mean[k] * inv_n255); }
    if (p.has_alpha) {                                                       // incremental PCA
        axis[0] = axis[1] = axis[2] = axis[3] = 0.0f;
        for (uint32_t i = first; i < 16; ++i) {
            if (!((p.mask >> i) & 1u)) continue;
            const uint32_t cc = bcast(px, i);
            float col[4], n[4], a[4], b[4], c[4], d[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) col[k] = (float)ch(cc, k) - mean_scaled[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) { a[k] = col[k] * col[0]; b[k] = col[k] * col[1]; c[k] = col[k] * col[2]; d[k] = col[k] * col[3]; }
#pragma unroll
            for (int k = 0; k < 4; ++k) n[k] = i != first ? axis[k] : col[k];
            normalize4(n);
            axis[0] += dot4(a, n); axis[1] += dot4(b, n); axis[2] += dot4(c, n); axis[3] += dot4(d, n);
        }
        normalize4(axis);
    } else {                                                                 // covariance and three power iterations
        float c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0;
        for (uint32_t i = first; i < 16; ++i) {
            if (!((p.mask >> i) & 1u)) continue;
            const uint32_t cc = bcast(px, i);
            const float rr = (float)ch(cc, 0) - mean_scaled[0], g = (float)ch(cc, 1) - mean_scaled[1], b = (float)ch(cc, 2) - mean_scaled[2];
            c0 += rr * rr; c1 += rr * g; c2 += rr * b; c3 += g * g; c4 += g * b; c5 += b * b;
        }
        float vfr = .9f, vfg = 1.0f, vfb = .7f;
#pragma unroll
        for (int iter = 0; iter < 3; ++iter) {
            float rr = vfr * c0 + vfg * c1 + vfb * c2;
            float g = vfr * c1 + vfg * c3 + vfb * c4;
            float b = vfr * c2 + vfg * c4 + vfb * c5;
            const float ar = fabsf(rr), ag = fabsf(g), ab = fabsf(b), m0 = ar > ag ? ar : ag;
            float m = m0 > ab ? m0 : ab;
            if (m > 1e-10f) { m = 1.0f / m; rr *= m; g *= m; b *= m; }
            vfr = rr; vfg = g; vfb = b;
        }
        float len = vfr * vfr + vfg * vfg + vfb * vfb;
        if (len < 1e-10f) axis[0] = axis[1] = axis[2] = axis[3] = 0.0f;
        else { len = 1.0f / sqrtf(len); vfr *= len; vfg *= len; vfb *= len; axis[0] = vfr; axis[1] = vfg; axis[2] = vfb; axis[3] = 0.0f; }
    }
    if (dot4(axis, axis) < .5f) {
        axis[0] = .213f; axis[1] = .715f; axis[2] = .072f; axis[3] = p.has_alpha ? .715f : 0.0f;
        normalize4(axis);
    }
    float l = 1e+9f, h = -1e+9f;
    for (uint32_t i = first; i < 16; ++i) {
        if (!((p.mask >> i) & 1u)) continue;
        const uint32_t cc = bcast(px, i);
        float q[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) q[k] = (float)ch(cc, k) - mean_scaled[k];
        const float d = dot4(q, axis);
        l = l < d ? l : d; h = h > d ? h : d;
    }
    l *= 1.0f / 255.0f; h *= 1.0f / 255.0f;
    float mn[4], mx[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) { const float b0 = axis[k] * l, b1 = axis[k] * h; mn[k] = saturate(mean[k] + b0); mx[k] = saturate(mean[k] + b1); }
    if (mn[0] + mn[1] + mn[2] + mn[3] > mx[0] + mx[1] + mx[2] + mx[3]) {
#pragma unroll
        for (int k = 0; k < 4; ++k) { const float s = mn[k]; mn[k] = mx[k]; mx[k] = s; }
    }
    if (!find_optimal_solution(p, mn, mx, r, px, mine, member)) return 0;
    {                                                                        // compute_least_squares_endpoints_rgb / _rgba
        const float (*wx)[4] = p.nw == 16 ? g_tab.wx4 : g_tab.wx3;
        float z00 = 0, z10 = 0, z11 = 0, q00[4] = { 0, 0, 0, 0 }, t[4] = { 0, 0, 0, 0 };
        for (uint32_t i = first; i < 16; ++i) {
            if (!((p.mask >> i) & 1u)) continue;
            const uint32_t cc = bcast(px, i), s = bcast(r.sel, i);
            z00 += wx[s][0]; z10 += wx[s][1]; z11 += wx[s][2];
            const float w = wx[s][3];
#pragma unroll
            for (int k = 0; k < 4; ++k) if (k < 3 || p.has_alpha) { q00[k] += w * (float)ch(cc, k); t[k] += (float)ch(cc, k); }
        }
        const float z01 = z10;
        float det = z00 * z11 - z01 * z10;
        if (det != 0.0f) det = 1.0f / det;
        const float iz00 = z11 * det, iz01 = -z01 * det, iz10 = -z10 * det, iz11 = z00 * det;
        float xl[4], xh[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float q10 = t[k] - q00[k];
            xl[k] = iz00 * q00[k] + iz01 * q10; xh[k] = iz10 * q00[k] + iz11 * q10;
        }
        if (!p.has_alpha) xl[3] = xh[3] = 255.0f;
#pragma unroll
        for (int k = 0; k < 4; ++k) { xl[k] = xl[k] * (1.0f / 255.0f); xh[k] = xh[k] * (1.0f / 255.0f); }
        if (!find_optimal_solution(p, xl, xh, r, px, mine, member)) return 0;
    }
    if (p.mode == 1) {                                                       // :1304-1318, the subset as its mean colour
        Res avg = r;                                                         // (mean is finite and in [0, 1]: the three are 0..255)
        const uint32_t cr = (uint32_t)f2i(.5f + mean[0] * 255.0f), cg = (uint32_t)f2i(.5f + mean[1] * 255.0f), cb = (uint32_t)f2i(.5f + mean[2] * 255.0f);
        const uint64_t e = pack_one_color(p, avg, cr & 255u, cg & 255u, cb & 255u, mine, member);
        if (e < r.best) { r = avg; r.sel = 2; r.best = e; }
    }
    return r.best;
}

// color_cell_compression_est (perceptual) in full for the pixels of `mask`; every lane has its own mask, pixel i comes from lane i
__device__ __forceinline__ uint64_t estimate_cell(uint32_t mask, uint32_t px)
{
    uint32_t lr = 255, lg = 255, lb = 255, hr = 0, hg = 0, hb = 0;
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t c = bcast(px, i);
        if ((mask >> i) & 1u) {
            lr = min(lr, ch(c, 0)); lg = min(lg, ch(c, 1)); lb = min(lb, ch(c, 2));
            hr = max(hr, ch(c, 0)); hg = max(hg, ch(c, 1)); hb = max(hb, ch(c, 2));
        }
    }
    const int ar = (int)hr - (int)lr, ag = (int)hg - (int)lg, ab = (int)hb - (int)lb;
    int dots[8], thresh[7];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t w = i == 0 ? 0u : i == 1 ? 9u : i == 2 ? 18u : i == 3 ? 27u : i == 4 ? 37u : i == 5 ? 46u : i == 6 ? 55u : 64u;
        dots[i] = (int)lerp64(lr, hr, w) * ar + (int)lerp64(lg, hg, w) * ag + (int)lerp64(lb, hb, w) * ab;
    }
#pragma unroll
    for (int i = 0; i < 7; ++i) thresh[i] = (dots[i] + dots[i + 1] + 1) >> 1;
    uint64_t total = 0;
    for (uint32_t i = 0; i < 16; ++i) {
        const uint32_t c = bcast(px, i);
        if (!((mask >> i) & 1u)) continue;
        const int d = ar * (int)ch(c, 0) + ag * (int)ch(c, 1) + ab * (int)ch(c, 2);
        uint32_t s = 0;                                                      // the thresholds do not decrease: the chain of :1388-1402 counts them
#pragma unroll
        for (int k = 0; k < 7; ++k) s += d >= thresh[k] ? 1u : 0u;
        const uint32_t w = (uint32_t)(0x40372E251B120900ull >> (8 * s)) & 255u;                 // g_bc7_weights3[s]
        const uint32_t e = dist_ycc(ycc(lerp64(lr, hr, w), lerp64(lg, hg, w), lerp64(lb, hb, w)), ycc(ch(c, 0), ch(c, 1), ch(c, 2)));
        total += (uint64_t)(int64_t)(int)e;
    }
    return total;
}

// estimate_partition: the scan's verdict from all 64 estimates
__device__ __forceinline__ uint32_t estimate_partition(uint32_t px, uint32_t li)
{
    uint64_t est[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const uint32_t m = kPart2[kOrder[s * 16 + li]];
        est[s] = estimate_cell(~m & 0xFFFFu, px) + estimate_cell(m, px);
    }
    uint64_t best_err = ~0ull;
    uint32_t best = 0, key = 0;
    bool done = false;
#pragma unroll
    for (int s = 0; s < 4; ++s)
        for (uint32_t l = 0; l < 16; ++l) {
            if (done || best_err == 0) { done = true; break; }
            const uint32_t it = (uint32_t)s * 16 + l, part = kOrder[it];
            if (it >= 14 && it <= 34 && !(kPredict[part] & (1u << (key + 1)))) {
                if (it == 34) { done = true; break; }
                continue;
            }
            const uint64_t e = bcast64(est[s], l);
            if (e < best_err) { best_err = e; best = part; }
            if (part == 34 && best != 34) { done = true; break; }
            if (it == 13) key = best;
        }
    return best;
}

struct BlockBits {
    uint64_t lo = 0, hi = 0; uint32_t ofs = 0;
    __device__ __forceinline__ void put(uint32_t v, uint32_t n)
    {
        if (ofs < 64) { lo |= (uint64_t)v << ofs; if (ofs + n > 64) hi |= (uint64_t)v >> (64 - ofs); }
        else hi |= (uint64_t)v << (ofs - 64);
        ofs += n;
    }
};

// bc7enc16_compress_block on the tile whose pixel li this lane holds; the block comes back in every lane
__device__ __forceinline__ void encode_tile(uint32_t px, uint32_t li, uint64_t* out_lo, uint64_t* out_hi)
{
    const Ycc mine = ycc(ch(px, 0), ch(px, 1), ch(px, 2));
    const bool alpha = tile_ballot(ch(px, 3) < 255u) != 0;
    Res r6{}, ra{}, rb{};
    uint32_t sel1 = 0, part = 0, pm = 0;
    uint64_t best = 0, trial = 0;
    bool tried = false;
    for (int pass = 0; pass < 3; ++pass) {                                   // mode 6, then the two subsets of mode 1
        Cell p;
        p.mode = pass == 0 ? 6u : 1u;
        p.mask = pass == 0 ? 0xFFFFu : pass == 1 ? ~pm & 0xFFFFu : pm;
        p.n = (uint32_t)__builtin_popcount(p.mask);
        p.nw = pass == 0 ? 16u : 8u; p.comp_bits = pass == 0 ? 7u : 6u;
        p.has_alpha = pass == 0 && alpha; p.share_pbit = pass != 0;
        const bool member = (p.mask >> li) & 1u;
        Res r;
        const uint64_t e = color_cell_compression(p, r, px, mine, member);
        if (pass == 0) {
            r6 = r; best = e;
            if (alpha || best == 0) break;
            tried = true;
            part = estimate_partition(px, li);
            pm = kPart2[part];
        } else {
            if (member) sel1 = r.sel;
            if (pass == 1) ra = r; else rb = r;
            trial += e;
            if (trial > best) break;
        }
    }
    BlockBits b;
    uint32_t sel, ofs;
    if (tried && trial < best) {                                             // encode_bc7_block, mode 1
        sel = sel1;
        const uint32_t anchor = kAnchor2[part];
        if (bcast(sel, 0) & 4u) { if (!((pm >> li) & 1u)) sel = 7u - sel; const uint32_t s = ra.lo; ra.lo = ra.hi; ra.hi = s; }
        if (bcast(sel, anchor) & 4u) { if ((pm >> li) & 1u) sel = 7u - sel; const uint32_t s = rb.lo; rb.lo = rb.hi; rb.hi = s; }
        b.put(2u, 2); b.put(part, 6);
#pragma unroll
        for (int c = 0; c < 3; ++c) { b.put(ch(ra.lo, c), 6); b.put(ch(ra.hi, c), 6); b.put(ch(rb.lo, c), 6); b.put(ch(rb.hi, c), 6); }
        b.put(ra.pb0, 1); b.put(rb.pb0, 1);
        ofs = 82u + 3u * li - (li > 0 ? 1u : 0u) - (li > anchor ? 1u : 0u);
    } else {                                                                 // mode 6
        sel = r6.sel;
        if (bcast(sel, 0) & 8u) { sel = 15u - sel; uint32_t s = r6.lo; r6.lo = r6.hi; r6.hi = s; s = r6.pb0; r6.pb0 = r6.pb1; r6.pb1 = s; }
        b.put(64u, 7);
#pragma unroll
        for (int c = 0; c < 4; ++c) { b.put(ch(r6.lo, c), 7); b.put(ch(r6.hi, c), 7); }
        b.put(r6.pb0, 1); b.put(r6.pb1, 1);
        ofs = 65u + 4u * li - (li > 0 ? 1u : 0u);
    }
    *out_lo = b.lo;
    *out_hi = b.hi | or16((uint64_t)sel << (ofs - 64u));                      // every selector lies in the upper half
}

// dword k of the 148 header bytes (dds.d:75-113); every other one is 0
__device__ __forceinline__ uint32_t header_dword(uint32_t k, uint32_t w, uint32_t h)
{
    switch (k) {
    case 0: return 0x20534444u;                                              // "DDS "
    case 1: return 124u;                                                     // dwSize
    case 2: return 0x81007u;                                                 // CAPS | HEIGHT | WIDTH | PIXELFORMAT | LINEARSIZE
    case 3: return h;
    case 4: return w;
    case 5: return (((w + 3u) & ~3u) * ((h + 3u) & ~3u) * 8u) >> 3;          // lPitch, in uint as the reference computes it
    case 19: return 32u;                                                     // ddpfPixelFormat.dwSize
    case 20: return 4u;                                                      // DDPF_FOURCC
    case 21: return 0x30315844u;                                             // "DX10"
    case 27: return 0x1000u;                                                 // DDSCAPS_TEXTURE
    case 32: return 98u;                                                     // DXGI_FORMAT_BC7_UNORM
    case 33: return 3u;                                                      // resourceDimension: TEXTURE2D
    case 35: return 1u;                                                      // arraySize
    default: return 0u;
    }
}

// imgs: tile t of the batch is tile t - tile0 of the image that owns it.  raw: 64 bytes per tile in, 16 bytes per tile out.
__global__ __launch_bounds__(kThreads) void k_bc7_encode(const EncImg* imgs, int n_img, uint32_t n_tiles, const uint8_t* raw, uint8_t* out)
{
    const uint32_t t = blockIdx.x * kTilesPerBlock + threadIdx.x / kLanes, li = threadIdx.x % kLanes;
    if (t >= n_tiles) return;                                                // (uniform over a tile's lanes; the kernel has no barrier)
    uint32_t px = 0;
    uint8_t* dst;
    if (raw) {
        const uint8_t* s = raw + (size_t)t * 64 + li * 4;
        px = s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (uint32_t)s[3] << 24;
        dst = out + (size_t)t * 16;
    } else {
        const EncImg im = imgs[find_unit<&EncImg::tile0>(imgs, n_img, t)];
        const uint32_t k = t - im.tile0, x = (k % im.bw) * 4 + (li & 3u), y = (k / im.bw) * 4 + (li >> 2);
        if (x < im.w && y < im.h) {                                          // dds.d:133-203; outside the image (0, 0, 0, 0)
            const uint8_t* s = im.src + (int64_t)y * im.pitch + (int64_t)x * im.comp;
            if (im.comp == 1) px = s[0] * 0x010101u | 0xFF000000u;
            else if (im.comp == 2) px = s[0] * 0x010101u | (uint32_t)s[1] << 24;
            else px = s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16 | (im.comp == 4 ? (uint32_t)s[3] << 24 : 0xFF000000u);
        }
        uint8_t* file = out + im.out_off;
        if (k == 0)
            for (uint32_t b = li; b < (uint32_t)kHeader; b += kLanes) file[b] = (uint8_t)(header_dword(b >> 2, im.w, im.h) >> (8 * (b & 3u)));
        dst = file + kHeader + (size_t)k * 16;
    }
    uint64_t lo, hi;
    encode_tile(px, li, &lo, &hi);
    if (((uintptr_t)dst & 3u) == 0) {
        if (li < 4) reinterpret_cast<uint32_t*>(dst)[li] = (uint32_t)((li < 2 ? lo : hi) >> (32 * (li & 1u)));
    } else {
        dst[li] = (uint8_t)((li < 8 ? lo : hi) >> (8 * (li & 7u)));
    }
}

int64_t encode_bound(int w, int h, int comp)
{
    if (comp < 1 || comp > 4 || w < 1 || h < 1) return 0;
    const int64_t b = kHeader + 16 * (((int64_t)w + 3) / 4) * (((int64_t)h + 3) / 4);
    return b > 0x7fffffffLL ? 0 : b;
}

float six_decimals(double x) { return (float)(floor(x * 1e6 + 0.5) / 1e6); }  // the reference's literals are the values to 6 decimals

// the tables, computed: for every value and p-bit the first (lo, hi) in lo-major order with the least squared error at weight
// index 2 (18 / 64); a strictly smaller error replaces
void compute_tables(Tables& t)
{
    static const uint32_t w3[8] = { 0, 9, 18, 27, 37, 46, 55, 64 }, w4[16] = { 0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64 };
    for (int k = 0; k < 24; ++k) {
        float* o = k < 8 ? t.wx3[k] : t.wx4[k - 8];
        const double w = (k < 8 ? w3[k] : w4[k - 8]) / 64.0;
        o[0] = six_decimals(w * w); o[1] = six_decimals((1 - w) * w); o[2] = six_decimals((1 - w) * (1 - w)); o[3] = six_decimals(w);
    }
    for (int c = 0; c < 256; ++c)
        for (uint32_t p = 0; p < 2; ++p) {
            int best = INT_MAX;
            for (uint32_t lo = 0; lo < 64; ++lo)
                for (uint32_t hi = 0; hi < 64; ++hi) {
                    uint32_t low = ((lo << 1) | p) << 1, high = ((hi << 1) | p) << 1;
                    low |= low >> 7; high |= high >> 7;
                    const int v = (int)((low * (64 - 18) + high * 18 + 32) >> 6), e = (v - c) * (v - c);
                    if (e < best) { best = e; t.opt1[c][p] = (uint32_t)e | lo << 16 | hi << 24; }
                }
        }
}

// once per device; the copy is synchronous, so every later launch on any stream sees the tables
int ensure_tables()
{
    static std::mutex mu;
    static std::vector<int> ready;
    static Tables host;
    static bool computed = false;
    std::lock_guard<std::mutex> lock(mu);
    const int dev = current_device();
    for (int d : ready) if (d == dev) return GAMUT_HIP_OK;
    if (!computed) { compute_tables(host); computed = true; }
    GAMUT_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_tab), &host, sizeof host));
    ready.push_back(dev);
    return GAMUT_HIP_OK;
}

// Measurements (tools/dds_encode_bench.py): with GAMUT_HIP_DDS_TIMING=1 an encode call brackets its launch with events and keeps
// the GPU time of the calling thread's last call.
thread_local float t_last_encode_ms[1] = { -1.0f };

int launch(const EncImg* dimg, int n_img, uint32_t n_tiles, const uint8_t* raw, uint8_t* out, hipStream_t stream)
{
    static const bool timing = env_flag("GAMUT_HIP_DDS_TIMING");
    KernelTimer<2> timer(timing);
    timer.mark(stream);
    hipLaunchKernelGGL(k_bc7_encode, dim3((n_tiles + kTilesPerBlock - 1) / kTilesPerBlock), dim3(kThreads), 0, stream, dimg, n_img, n_tiles, raw, out);
    if (int rc = launch_status("dds_encode")) return rc;
    timer.mark(stream);
    GAMUT_HIP_CHECK(hipStreamSynchronize(stream));
    timer.finish(t_last_encode_ms);
    return GAMUT_HIP_OK;
}

int encode_batch(const uint8_t* const* src, const int64_t* src_pitch, const int32_t* width, const int32_t* height, const int32_t* comp, int count,
                 const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host, hipStream_t stream)
{
    std::vector<EncImg> imgs; std::vector<int> which;
    int first_bad = -1;
    uint64_t tiles = 0;
    for (int i = 0; i < count; ++i) {
        out_len[i] = 0;
        const bool ok = encode_bound(width[i], height[i], comp[i]) > 0 && src[i] && out_offset[i] >= 0;
        if (status_host) status_host[i] = ok ? GAMUT_HIP_OK : GAMUT_HIP_ERR_INVALID_ARG;
        if (!ok) { if (first_bad < 0) first_bad = i; continue; }
        EncImg im{};
        im.src = src[i]; im.pitch = src_pitch[i]; im.out_off = out_offset[i];
        im.w = (uint32_t)width[i]; im.h = (uint32_t)height[i]; im.bw = (im.w + 3) / 4; im.comp = (uint32_t)comp[i];
        im.tile0 = (uint32_t)tiles;
        tiles += (uint64_t)im.bw * ((im.h + 3) / 4);
        if (tiles > 0x7FFFFFFFull) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "dds_encode: batch of more than 2^31 tiles");
        imgs.push_back(im); which.push_back(i);
    }
    if (!imgs.empty()) {
        if (int rc = ensure_tables()) return rc;
        const int n = (int)imgs.size();
        const size_t bytes = (size_t)n * sizeof(EncImg);
        static thread_local PerDevice<DeviceScratch> scratch_pd;
        static thread_local PerDevice<PinnedScratch> pinned_pd;
        uint8_t* d = (uint8_t*)scratch_pd.cur().get(bytes, stream);
        uint8_t* h = pinned_pd.cur().get(bytes, stream);
        if (!d || !h) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "dds_encode: scratch allocation of %zu bytes failed", bytes);
        memcpy(h, imgs.data(), bytes);
        GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, stream));
        if (int rc = launch((const EncImg*)d, n, (uint32_t)tiles, nullptr, out, stream)) { (void)hipStreamSynchronize(stream); return rc; }
        for (int k = 0; k < n; ++k) out_len[which[(size_t)k]] = encode_bound((int)imgs[(size_t)k].w, (int)imgs[(size_t)k].h, (int)imgs[(size_t)k].comp);
    }
    if (first_bad >= 0) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "image %d: dds_encode: refused shape or source", first_bad);
    return GAMUT_HIP_OK;
}

} // namespace
} // namespace gamut

using namespace gamut;

extern "C" {

int64_t gamut_hip_dds_encode_bound(int width, int height, int comp) { return encode_bound(width, height, comp); }

int gamut_hip_dds_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const int32_t* width, const int32_t* height,
                                      const int32_t* comp, int count, const int64_t* out_offset, uint8_t* out, int64_t* out_len,
                                      int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!src || !src_pitch || !width || !height || !comp || !out_offset || !out || !out_len)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "dds_encode_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return encode_batch(src, src_pitch, width, height, comp, count, out_offset, out, out_len, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "dds_encode_batch_device: out of host memory");
    }
}

int gamut_hip_bc7_encode_blocks_device(const uint8_t* rgba_tiles, int64_t n, uint8_t* out, void* stream)
{
    clear_error();
    if (n < 0 || n > 0x7FFFFFFFLL || (n > 0 && (!rgba_tiles || !out))) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "bc7_encode_blocks_device: bad arguments");
    if (n == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        if (int rc = ensure_tables()) return rc;
        return launch(nullptr, 0, (uint32_t)n, rgba_tiles, out, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "bc7_encode_blocks_device: out of host memory");
    }
}

void* gamut_hip_dds_write_to_mem(const void* data, int pitch, int w, int h, int comp, int* out_len)
{
    clear_error();
    if (!data || !out_len || encode_bound(w, h, comp) == 0) {
        set_error(GAMUT_HIP_ERR_INVALID_ARG, "dds_write_to_mem: invalid arguments"); return nullptr;
    }
    if (!have_device()) return nullptr;
    const int32_t W = w, H = h, Cc = comp;
    return encode_host_image("dds_write_to_mem", HostRows{ data, pitch, (size_t)w * comp, h, 1, 0 }, (size_t)encode_bound(w, h, comp), out_len,
        [&](const uint8_t* src, int64_t spitch, int64_t, int64_t off, uint8_t* d, int64_t* n, hipStream_t st) {
            int status = 0;
            return encode_batch(&src, &spitch, &W, &H, &Cc, 1, &off, d, n, &status, st);
        });
}

float gamut_hip_dds_last_encode_kernel_ms(void) { return t_last_encode_ms[0]; }

} // extern "C"
