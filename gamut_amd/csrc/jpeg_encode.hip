// jpeg_encode.hip -- baseline JPEG encode on the GPU: the bytes of stbi_write_jpg_core (codecs/stb_image_write.d:632-880), many
// images per batch.
//
// Every block's coefficients and every block's AC bits depend on that block alone; only the DC difference (three predictors: Y, U,
// V), the bit positions and the 0xFF stuffing are sequential, and each becomes a prefix sum.  Five plain launches per chunk of
// images, no workgroup ever waits for another:
//   1. k_jenc_fdct  : one wave per 8x8 block, lane = coefficient.  Gather with edge clamping, colour conversion (4:2:0: the 2x2
//                     average), AAN float DCT (rows, LDS transpose, columns), quantisation, zig-zag.  Stores the int16
//                     coefficients, the DC and the block's AC bit count (run lengths from a ballot over the non-zero lanes).
//   2. k_jenc_scan  : one workgroup per image: DC-difference bits from the predecessor's DC, exclusive scan -> each block's bit
//                     offset in the image's raw (unstuffed) stream and its length T; zeroes the raw words that blocks share.
//   3. k_jenc_emit  : one wave per block: every lane's codes, a lane scan places them, the block is assembled in LDS and stored
//                     (words it shares with a neighbour by atomicOr, the others plainly); the last block adds the 7 fill bits.
//   4. k_jenc_count : the 0xFF bytes of each 4 KB chunk of the raw stream, per workgroup range;
//   5. k_jenc_stuff : the bytes with a 0x00 after every 0xFF, at offsets from the counts; header, EOI and the stream length.
// Raw streams are 32-bit words holding their bits MSB first (the first bit of the stream is bit 31 of word 0).
// The float arithmetic is the reference's operation for operation: the library is built with -ffp-contract=off -fno-fast-math,
// and nothing here uses an fma builtin.  The quantiser reciprocals (fdtbl) come from the host.
#include "encode_host.hpp"
#include "device_util.hpp"

namespace gamut {
namespace {

constexpr int kHeader = 607;                          // SOI + APP0 + DQT + SOF0 + DHT + SOS (stb_image_write.d:796-817)
constexpr int kMaxBlockBits = 1660;                   // DC <= 11 + 11 bits; 63 AC lanes each <= 16 + 10 bits (ZRLs replace zeros)
constexpr int kMaxDim = 65535;                        // SOF0 holds 16-bit sizes (a deliberate refusal: the reference would truncate)
constexpr uint32_t kChunkBlocks = 1u << 22;           // blocks per launch set: scratch ~350 B per block
constexpr size_t kChunkImages = 16384;                // images per launch set (grid.y of the stuffing passes)
constexpr int kStuffChunk = 4096;                     // bytes per stuffing step (256 threads x 16 bytes)

const uint8_t kZigzag[64] = {
    0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63 };
__constant__ uint8_t c_zigzag[64] = {
    0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63 };

// ITU T.81 Annex K: quantisation tables K.1 / K.2 (natural order), Huffman BITS / HUFFVAL of K.3-K.6
const int kLumaQ[64] = { 16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
    14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
    49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99 };
const int kChromaQ[64] = { 17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
    47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
    99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99 };
const uint8_t kDcBits[2][16] = { { 0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0 }, { 0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0 } };
const uint8_t kDcVals[12] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11 };
const uint8_t kAcBits[2][16] = { { 0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d }, { 0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77 } };
const uint8_t kAcVals[2][162] = {
  { 0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5,
    0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9,
    0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa },
  { 0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
    0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
    0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
    0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
    0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa } };

// Huffman codes by symbol, code | length << 16 (length 0: a symbol the table does not have -- looked up by index all the same,
// as HTAC[(run << 4) + category] does); class 0 = luma, 1 = chroma
struct JHuff { uint32_t dc[2][16]; uint32_t ac[2][256]; };
// one per distinct (clamped quality, subsampling) of a batch: the quantiser reciprocals and the 607-byte header with zero sizes
struct JQual { float fd[2][64]; uint8_t hdr[608]; };
struct JImg {
    const uint8_t* src; int64_t pitch; int64_t out_off; uint64_t raw_w0;   // raw_w0: first word of the image's raw stream (multiple of 4)
    uint32_t w, h, comp, sub, q, mcux, blk0, nblk;                          // blocks [blk0, blk0 + nblk) of the chunk
};

// ---- device helpers ----------------------------------------------------------------------------------------------------------------
// block b of an image -> (class, MCU, position in the MCU).  4:2:0: Y(0,0) Y(8,0) Y(0,8) Y(8,8) U V; 4:4:4: Y U V
__device__ __forceinline__ void jblock_pos(const JImg& im, uint32_t b, uint32_t& mcu, uint32_t& p)
{
    const uint32_t per = im.sub ? 6u : 3u;
    mcu = b / per; p = b - mcu * per;
}
__device__ __forceinline__ int jblock_class(const JImg& im, uint32_t p) { return im.sub ? (p >= 4) : (p >= 1); }
// the block before b with the same DC predictor, or -1
__device__ __forceinline__ int64_t jblock_pred(const JImg& im, uint32_t b)
{
    uint32_t mcu, p; jblock_pos(im, b, mcu, p);
    if (im.sub) {
        if (p >= 1 && p <= 3) return (int64_t)b - 1;
        return mcu ? (int64_t)b - (p == 0 ? 3 : 6) : -1;
    }
    return mcu ? (int64_t)b - 3 : -1;
}

struct RGB { float r, g, b; };
__device__ __forceinline__ RGB jpix(const JImg& im, uint32_t x, uint32_t y)
{
    x = min(x, im.w - 1); y = min(y, im.h - 1);
    const uint8_t* q = im.src + (int64_t)y * im.pitch + (int64_t)x * im.comp;
    const int og = im.comp > 2 ? 1 : 0, ob = im.comp > 2 ? 2 : 0;
    return RGB{ (float)q[0], (float)q[og], (float)q[ob] };
}
__device__ __forceinline__ float jY(RGB c) { return 0.29900f * c.r + 0.58700f * c.g + 0.11400f * c.b - 128; }
__device__ __forceinline__ float jU(RGB c) { return -0.16874f * c.r - 0.33126f * c.g + 0.50000f * c.b; }
__device__ __forceinline__ float jV(RGB c) { return 0.50000f * c.r - 0.41869f * c.g - 0.08131f * c.b; }

// stbiw__jpg_DCT on d0..d7, output j (every statement in the reference's order; the caller reads the 8 inputs from LDS)
__device__ __forceinline__ float jdct_pick(const float* d, int s, int j)
{
    const float d0 = d[0], d1 = d[s], d2 = d[2 * s], d3 = d[3 * s], d4 = d[4 * s], d5 = d[5 * s], d6 = d[6 * s], d7 = d[7 * s];
    const float t0 = d0 + d7, t7 = d0 - d7, t1 = d1 + d6, t6 = d1 - d6, t2 = d2 + d5, t5 = d2 - d5, t3 = d3 + d4, t4 = d3 - d4;
    const float t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    const float o0 = t10 + t11, o4 = t10 - t11;
    const float z1 = (t12 + t13) * 0.707106781f;
    const float o2 = t13 + z1, o6 = t13 - z1;
    const float u10 = t4 + t5, u11 = t5 + t6, u12 = t6 + t7;
    const float z5 = (u10 - u12) * 0.382683433f;
    const float z2 = u10 * 0.541196100f + z5;
    const float z4 = u12 * 1.306562965f + z5;
    const float z3 = u11 * 0.707106781f;
    const float z11 = t7 + z3, z13 = t7 - z3;
    const float o5 = z13 + z2, o3 = z13 - z2, o1 = z11 + z4, o7 = z11 - z4;
    float r = o0;
    r = j == 1 ? o1 : r; r = j == 2 ? o2 : r; r = j == 3 ? o3 : r; r = j == 4 ? o4 : r;
    r = j == 5 ? o5 : r; r = j == 6 ? o6 : r; r = j == 7 ? o7 : r;
    return r;
}

__device__ __forceinline__ uint32_t jcat(int v) { const uint32_t a = (uint32_t)(v < 0 ? -v : v); return a ? 32u - __clz(a) : 1u; }
__device__ __forceinline__ uint32_t jvbits(int v, uint32_t n) { return (uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1u); }

// the AC codes lane `lane` (1..63) emits for its coefficient v (zig-zag order): ZRLs, (run, size) code, magnitude bits, and the EOB
// when this is the last non-zero coefficient and it is not at 63.  `nz` = ballot of the non-zero lanes 1..63.  Lane 0 gets nothing.
__device__ __forceinline__ void jac_lane(const JHuff* hf, int cls, int lane, int v, uint64_t nz, uint64_t& bits, uint32_t& n)
{
    bits = 0; n = 0;
    if (lane == 0 || v == 0) return;
    const uint64_t below = nz & ((1ull << lane) - 1ull);
    const int prev = below ? 63 - __clzll(below) : 0;
    int zeros = lane - prev - 1;
    const uint32_t zrl = hf->ac[cls][0xF0];
    for (; zeros >= 16; zeros -= 16) { bits = bits << (zrl >> 16) | (zrl & 0xFFFFu); n += zrl >> 16; }
    const uint32_t cat = jcat(v), e = hf->ac[cls][((zeros << 4) + cat) & 255];
    bits = bits << (e >> 16) | (e & 0xFFFFu); n += e >> 16;
    bits = bits << cat | jvbits(v, cat); n += cat;
    const int end = 63 - __clzll(nz);
    if (lane == end && end != 63) { const uint32_t eob = hf->ac[cls][0]; bits = bits << (eob >> 16) | (eob & 0xFFFFu); n += eob >> 16; }
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v)
{
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane)
{
    for (int d = 1; d < 64; d <<= 1) { const uint32_t u = __shfl_up(v, d, 64); if (lane >= d) v += u; }
    return v;
}

constexpr int kWaves = 4;                             // waves (= blocks in flight) per workgroup of the per-block kernels

// ---- 1. forward transform --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kWaves) void k_jenc_fdct(const JImg* imgs, int n_img, uint32_t n_blk, const JQual* quals, const JHuff* hf,
                                                          int16_t* coef, int32_t* dc, uint32_t* acb)
{
    __shared__ float buf[kWaves][2][64];
    __shared__ int du[kWaves][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane >> 3, c = lane & 7;
    const uint32_t groups = (n_blk + kWaves - 1) / kWaves;
    for (uint32_t gi = blockIdx.x; gi < groups; gi += gridDim.x) {    // uniform over the workgroup: the barriers below are safe
        const uint32_t g = gi * kWaves + wave;
        const bool live = g < n_blk;
        JImg im{}; uint32_t mcu = 0, p = 0; int cls = 0;
        if (live) {
            im = imgs[find_unit<&JImg::blk0>(imgs, n_img, g)];
            jblock_pos(im, g - im.blk0, mcu, p);
            cls = jblock_class(im, p);
            const uint32_t my = mcu / im.mcux, mx = mcu - my * im.mcux;
            float s;
            if (im.sub) {
                const uint32_t x0 = mx * 16, y0 = my * 16;
                if (p < 4) {
                    s = jY(jpix(im, x0 + (p & 1) * 8 + c, y0 + (p >> 1) * 8 + r));
                } else {
                    const uint32_t x = x0 + 2 * c, y = y0 + 2 * r;
                    const RGB a = jpix(im, x, y), b = jpix(im, x + 1, y), e = jpix(im, x, y + 1), f = jpix(im, x + 1, y + 1);
                    s = p == 4 ? (jU(a) + jU(b) + jU(e) + jU(f)) * 0.25f : (jV(a) + jV(b) + jV(e) + jV(f)) * 0.25f;
                }
            } else {
                const RGB a = jpix(im, mx * 8 + c, my * 8 + r);
                s = p == 0 ? jY(a) : p == 1 ? jU(a) : jV(a);
            }
            buf[wave][0][lane] = s;
        }
        __syncthreads();
        if (live) buf[wave][1][lane] = jdct_pick(&buf[wave][0][r * 8], 1, c);          // rows
        __syncthreads();
        if (live) {
            const float v = jdct_pick(&buf[wave][1][c], 8, r) * quals[im.q].fd[cls][lane];   // columns, then quantise
            du[wave][c_zigzag[lane]] = (int)(v < 0 ? v - 0.5f : v + 0.5f);
        }
        __syncthreads();
        if (live) {
            const int v = du[wave][lane];                                                 // lane = zig-zag position
            coef[(size_t)g * 64 + lane] = (int16_t)v;
            const uint64_t nz = __ballot(v != 0) & ~1ull;
            uint64_t bits; uint32_t n;
            jac_lane(hf, cls, lane, v, nz, bits, n);
            if (lane == 0 && nz == 0) n = hf->ac[cls][0] >> 16;                          // EOB right after the DC
            n = wave_sum(n);
            if (lane == 0) { dc[g] = v; acb[g] = n; }
        }
    }
}

// ---- 2. per-image scan: DC bits, bit offsets, T ---------------------------------------------------------------------------------
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void k_jenc_scan(const JImg* imgs, const JHuff* hf, const int32_t* dc, const uint32_t* acb,
                                                           uint64_t* off, uint64_t* tbits, uint32_t* raw)
{
    __shared__ uint64_t part[kScanThreads / 64];
    const JImg im = imgs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t per = (im.nblk + kScanThreads - 1) / kScanThreads, b0 = min(im.nblk, tid * per), b1 = min(im.nblk, b0 + per);
    auto bits_of = [&](uint32_t b) -> uint64_t {
        const int64_t pb = jblock_pred(im, b);
        const int diff = dc[im.blk0 + b] - (pb >= 0 ? dc[im.blk0 + pb] : 0);
        uint32_t mcu, p; jblock_pos(im, b, mcu, p);
        const uint32_t cat = diff ? jcat(diff) : 0u;
        return (uint64_t)acb[im.blk0 + b] + (hf->dc[jblock_class(im, p)][cat] >> 16) + cat;
    };
    uint64_t s = 0;
    for (uint32_t b = b0; b < b1; ++b) s += bits_of(b);
    uint64_t incl = s;                                                      // scan over the workgroup: waves, then wave totals
    for (int d = 1; d < 64; d <<= 1) { const uint64_t u = __shfl_up(incl, d, 64); if (lane >= d) incl += u; }
    if (lane == 63) part[wave] = incl;
    __syncthreads();
    uint64_t before = 0, total = 0;
    for (int k = 0; k < kScanThreads / 64; ++k) { if (k < wave) before += part[k]; total += part[k]; }
    uint64_t at = before + incl - s;
    uint32_t* rw = raw + im.raw_w0;
    for (uint32_t b = b0; b < b1; ++b) {
        off[im.blk0 + b] = at;
        rw[at >> 5] = 0u;                                                   // a word holding a block's start may be shared: cleared for atomicOr
        at += bits_of(b);
    }
    if (tid == 0) {
        rw[total >> 5] = 0u; rw[(total + 6) >> 5] = 0u;                    // the words the fill bits reach
        tbits[blockIdx.x] = total;
    }
}

// ---- 3. emit ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64 * kWaves) void k_jenc_emit(const JImg* imgs, int n_img, uint32_t n_blk, const JHuff* hf, const int16_t* coef,
                                                          const int32_t* dc, const uint64_t* off, const uint64_t* tbits, uint32_t* raw)
{
    __shared__ uint32_t words[kWaves][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t groups = (n_blk + kWaves - 1) / kWaves;
    for (uint32_t gi = blockIdx.x; gi < groups; gi += gridDim.x) {
        const uint32_t g = gi * kWaves + wave;
        const bool live = g < n_blk;
        words[wave][lane] = 0u;
        __syncthreads();
        uint64_t B = 0; uint32_t nw = 0, span = 0; int ii = 0;
        if (live) {
            ii = find_unit<&JImg::blk0>(imgs, n_img, g);
            const JImg& im = imgs[ii];
            const uint32_t b = g - im.blk0;
            uint32_t mcu, p; jblock_pos(im, b, mcu, p);
            const int cls = jblock_class(im, p);
            const int v = coef[(size_t)g * 64 + lane];
            const uint64_t nz = __ballot(v != 0) & ~1ull;
            uint64_t bits; uint32_t n;
            jac_lane(hf, cls, lane, v, nz, bits, n);
            if (lane == 0) {
                const int64_t pb = jblock_pred(im, b);
                const int diff = v - (pb >= 0 ? dc[im.blk0 + pb] : 0);
                const uint32_t cat = diff ? jcat(diff) : 0u, e = hf->dc[cls][cat];
                bits = e & 0xFFFFu; n = e >> 16;
                if (cat) { bits = bits << cat | jvbits(diff, cat); n += cat; }
                if (nz == 0) { const uint32_t eob = hf->ac[cls][0]; bits = bits << (eob >> 16) | (eob & 0xFFFFu); n += eob >> 16; }
            }
            const uint32_t incl = wave_incl_scan(n, lane), total = __shfl(incl, 63, 64);
            B = im.raw_w0 * 32 + off[g];
            const uint32_t lp = (uint32_t)(B & 31u) + incl - n;             // bit position inside the block's word window
            nw = ((uint32_t)(B & 31u) + total + 31) >> 5;
            span = total;
            if (n) {
                const uint32_t o = lp & 31, t = o + n, w0 = lp >> 5;        // t <= 31 + 63
                uint32_t x0, x1, x2 = 0;
                if (t <= 64) { const uint64_t x = bits << (64 - t); x0 = (uint32_t)(x >> 32); x1 = (uint32_t)x; }
                else { x2 = (uint32_t)(bits << (96 - t)); const uint64_t x = bits >> (t - 64); x0 = (uint32_t)(x >> 32); x1 = (uint32_t)x; }
                if (w0 < 64 && x0) atomicOr(&words[wave][w0], x0);
                if (w0 + 1 < 64 && x1) atomicOr(&words[wave][w0 + 1], x1);
                if (w0 + 2 < 64 && x2) atomicOr(&words[wave][w0 + 2], x2);
            }
        }
        __syncthreads();
        if (live) {
            uint32_t* rw = raw + (B >> 5);
            const uint32_t w = words[wave][lane];
            // a word is shared when the previous block ends in it (the block starts inside it) or the next block / the fill bits
            // start in it (the block ends inside it); k_jenc_scan cleared exactly those words.  Every other word is this block's alone.
            const bool shared = (lane == 0 && (B & 31u) != 0) || ((uint32_t)lane == nw - 1 && ((B + span) & 31u) != 0);
            if ((uint32_t)lane < nw && nw <= 64) {
                if (shared) { if (w) atomicOr(&rw[lane], w); }
                else rw[lane] = w;
            }
            const JImg& im = imgs[ii];
            if (lane == 0 && g == im.blk0 + im.nblk - 1) {                  // the fill bits 0x7F after the last block
                const uint64_t T = im.raw_w0 * 32 + tbits[ii];
                const uint64_t x = (uint64_t)0x7Fu << (57 - (T & 31));
                atomicOr(&raw[T >> 5], (uint32_t)(x >> 32));
                if ((uint32_t)x) atomicOr(&raw[(T >> 5) + 1], (uint32_t)x);
            }
        }
        __syncthreads();
    }
}

// ---- 4./5. stuffing -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void jchunk_range(uint64_t T, uint32_t G, uint32_t x, uint64_t& nbytes, uint64_t& c0, uint64_t& c1)
{
    nbytes = (T + 7) >> 3;
    const uint64_t nch = (nbytes + kStuffChunk - 1) / kStuffChunk, per = (nch + G - 1) / G;
    c0 = min(nch, (uint64_t)x * per); c1 = min(nch, c0 + per);
}
// the 16 bytes thread t covers of chunk ch, as a 128-bit group, and how many of them are 0xFF data bytes
__device__ __forceinline__ uint4 jchunk_load(const uint32_t* rw, uint64_t ch, int t, uint64_t nbytes, uint32_t& ff)
{
    const uint64_t i0 = ch * kStuffChunk + (uint64_t)t * 16;
    uint4 q = make_uint4(0, 0, 0, 0);
    ff = 0;
    if (i0 >= nbytes) return q;
    q = *reinterpret_cast<const uint4*>(rw + (i0 >> 2));
    const uint32_t wv[4] = { q.x, q.y, q.z, q.w };
    #pragma unroll
    for (int k = 0; k < 16; ++k)
        ff += (i0 + k < nbytes && ((wv[k >> 2] >> (24 - 8 * (k & 3))) & 255u) == 255u) ? 1u : 0u;
    return q;
}
constexpr int kStuffThreads = 256;
__global__ __launch_bounds__(kStuffThreads) void k_jenc_count(const JImg* imgs, const uint64_t* tbits, const uint32_t* raw, uint32_t* cnt)
{
    __shared__ uint32_t part[kStuffThreads / 64];
    const uint32_t G = gridDim.x, x = blockIdx.x, img = blockIdx.y;
    const int t = threadIdx.x;
    uint64_t nbytes, c0, c1; jchunk_range(tbits[img], G, x, nbytes, c0, c1);
    const uint32_t* rw = raw + imgs[img].raw_w0;
    uint32_t s = 0;
    for (uint64_t ch = c0; ch < c1; ++ch) { uint32_t ff; (void)jchunk_load(rw, ch, t, nbytes, ff); s += ff; }
    s = wave_sum(s);
    if ((t & 63) == 0) part[t >> 6] = s;
    __syncthreads();
    if (t == 0) cnt[(size_t)img * G + x] = part[0] + part[1] + part[2] + part[3];
}

__global__ __launch_bounds__(kStuffThreads) void k_jenc_stuff(const JImg* imgs, const JQual* quals, const uint64_t* tbits, const uint32_t* raw,
                                                              const uint32_t* cnt, uint8_t* out, int64_t* out_len)
{
    __shared__ uint32_t part[kStuffThreads / 64];
    const uint32_t G = gridDim.x, x = blockIdx.x, img = blockIdx.y;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const JImg& im = imgs[img];
    uint64_t nbytes, c0, c1; jchunk_range(tbits[img], G, x, nbytes, c0, c1);
    uint64_t carry = 0, all = 0;
    for (uint32_t k = 0; k < G; ++k) { const uint32_t v = cnt[(size_t)img * G + k]; if (k < x) carry += v; all += v; }
    const uint32_t* rw = raw + im.raw_w0;
    uint8_t* o = out + im.out_off;
    for (uint64_t ch = c0; ch < c1; ++ch) {
        uint32_t ff; const uint4 q = jchunk_load(rw, ch, t, nbytes, ff);
        const uint32_t incl = wave_incl_scan(ff, lane);
        if (lane == 63) part[wave] = incl;
        __syncthreads();
        uint32_t before = 0, tot = 0;
        for (int k = 0; k < kStuffThreads / 64; ++k) { if (k < wave) before += part[k]; tot += part[k]; }
        const uint64_t i0 = ch * kStuffChunk + (uint64_t)t * 16;
        uint64_t at = kHeader + i0 + carry + before + incl - ff;
        const uint32_t wv[4] = { q.x, q.y, q.z, q.w };
        for (int k = 0; k < 16 && i0 + k < nbytes; ++k) {
            const uint8_t byte = (uint8_t)(wv[k >> 2] >> (24 - 8 * (k & 3)));
            o[at++] = byte;
            if (byte == 0xFF) o[at++] = 0;
        }
        carry += tot;
        __syncthreads();
    }
    if (x == 0) {
        const uint8_t* hdr = quals[im.q].hdr;
        for (int k = t; k < kHeader; k += kStuffThreads) {
            uint8_t v = hdr[k];
            v = k == 159 ? (uint8_t)(im.h >> 8) : k == 160 ? (uint8_t)im.h : k == 161 ? (uint8_t)(im.w >> 8) : k == 162 ? (uint8_t)im.w : v;
            o[k] = v;
        }
        if (t == 0) {
            const uint64_t end = kHeader + nbytes + all;
            o[end] = 0xFF; o[end + 1] = 0xD9;
            out_len[img] = (int64_t)(end + 2);
        }
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// quality handling of stbi_write_jpg_core (stb_image_write.d:762-767): 0 means 90; 4:2:0 decided BEFORE the clamp
void jquality(int quality, int& scale, int& sub)
{
    quality = quality ? quality : 90;
    sub = quality <= 90 ? 1 : 0;
    quality = quality < 1 ? 1 : quality > 100 ? 100 : quality;
    scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
}
bool jvalid(int w, int h, int comp) { return w >= 1 && h >= 1 && w <= kMaxDim && h <= kMaxDim && comp >= 1 && comp <= 4; }
uint64_t jblocks(int w, int h, int sub)
{
    return sub ? 6ull * ((uint64_t)(w + 15) / 16) * ((uint64_t)(h + 15) / 16) : 3ull * ((uint64_t)(w + 7) / 8) * ((uint64_t)(h + 7) / 8);
}
// The stream is the header, ceil(T / 8) data bytes, one 0x00 per 0xFF data byte, and EOI.  T <= blocks * kMaxBlockBits: the DC of a
// block is at most an 11-bit code and 11 magnitude bits (its difference is below 2^11 in magnitude, DC values being below 2^10), and
// each of the 63 AC positions emits at most one 16-bit code and 10 magnitude bits (coefficients of 8-bit samples stay below 2^10);
// 16 zeros cost one 11-bit ZRL instead of 16 x 26 bits and the EOB only follows when fewer than 63 coefficients were coded.  So
// 22 + 63 * 26 = 1660 bits; stuffing at most doubles the data bytes.
int64_t jbound(int w, int h, int comp, int quality)
{
    if (!jvalid(w, h, comp)) return 0;
    int scale, sub; jquality(quality, scale, sub);
    const uint64_t blk = jblocks(w, h, sub);
    return (int64_t)(kHeader + 2 * ((blk * kMaxBlockBits + 7) / 8) + 2);
}

void jhuff_build(uint32_t* t, int n, const uint8_t* bits, const uint8_t* vals)    // T.81 C.2: canonical codes by length
{
    for (int i = 0; i < n; ++i) t[i] = 0;
    uint32_t code = 0; int k = 0;
    for (int l = 1; l <= 16; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k) t[vals[k]] = code++ | (uint32_t)l << 16;
        code <<= 1;
    }
}
const JHuff& jhuff()
{
    static const JHuff h = [] {
        JHuff x{};
        for (int c = 0; c < 2; ++c) { jhuff_build(x.dc[c], 16, kDcBits[c], kDcVals); jhuff_build(x.ac[c], 256, kAcBits[c], kAcVals[c]); }
        return x;
    }();
    return h;
}

void jqual_build(JQual& q, int scale, int sub)
{
    static const float s = 2.828427125f;
    static const float aasf[8] = { 1.0f * s, 1.387039845f * s, 1.306562965f * s, 1.175875602f * s, 1.0f * s, 0.785694958f * s,
                                   0.541196100f * s, 0.275899379f * s };
    uint8_t tab[2][64];
    for (int i = 0; i < 64; ++i) {
        const int a = (kLumaQ[i] * scale + 50) / 100, b = (kChromaQ[i] * scale + 50) / 100;
        tab[0][kZigzag[i]] = (uint8_t)(a < 1 ? 1 : a > 255 ? 255 : a);
        tab[1][kZigzag[i]] = (uint8_t)(b < 1 ? 1 : b > 255 ? 255 : b);
    }
    for (int c = 0; c < 2; ++c)
        for (int r = 0, k = 0; r < 8; ++r)
            for (int col = 0; col < 8; ++col, ++k) q.fd[c][k] = 1 / ((float)tab[c][kZigzag[k]] * aasf[r] * aasf[col]);
    uint8_t* h = q.hdr; int n = 0;
    auto put = [&](int v) { h[n++] = (uint8_t)v; };
    const uint8_t app0[20] = { 0xFF, 0xD8, 0xFF, 0xE0, 0, 0x10, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0 };
    for (int i = 0; i < 20; ++i) put(app0[i]);
    put(0xFF); put(0xDB); put(0); put(0x84);
    put(0); for (int i = 0; i < 64; ++i) put(tab[0][i]);
    put(1); for (int i = 0; i < 64; ++i) put(tab[1][i]);
    const uint8_t sof[19] = { 0xFF, 0xC0, 0, 0x11, 8, 0, 0, 0, 0, 3, 1, (uint8_t)(sub ? 0x22 : 0x11), 0, 2, 0x11, 1, 3, 0x11, 1 };  // sizes: 159-162
    for (int i = 0; i < 19; ++i) put(sof[i]);
    put(0xFF); put(0xC4); put(0x01); put(0xA2);
    for (int c = 0; c < 2; ++c) {
        put(c); for (int i = 0; i < 16; ++i) put(kDcBits[c][i]); for (int i = 0; i < 12; ++i) put(kDcVals[i]);
        put(0x10 | c); for (int i = 0; i < 16; ++i) put(kAcBits[c][i]); for (int i = 0; i < 162; ++i) put(kAcVals[c][i]);
    }
    const uint8_t sos[14] = { 0xFF, 0xDA, 0, 0x0C, 3, 1, 0, 2, 0x11, 3, 0x11, 0, 0x3F, 0 };
    for (int i = 0; i < 14; ++i) put(sos[i]);
    h[n] = 0;                                                          // n == kHeader
}

// one chunk of valid images: all five launches, then the lengths come back
int jencode_chunk(std::vector<JImg>& imgs, const std::vector<JQual>& quals, const std::vector<int>& which, int64_t* out_len,
                  uint8_t* out, hipStream_t stream)
{
    const int n = (int)imgs.size();
    uint64_t nb = 0, rw = 0;
    for (JImg& im : imgs) {
        im.blk0 = (uint32_t)nb; im.raw_w0 = rw;
        nb += im.nblk;
        rw += ((uint64_t)im.nblk * kMaxBlockBits + 7 + 31) / 32 + 2;          // + the word the fill bits may reach
        rw = (rw + 3) & ~3ull;                                                 // 16-byte loads in the stuffing passes
    }
    const uint32_t G = (uint32_t)std::max(1, std::min(64, 8192 / n));
    const size_t o_img = 0, o_q = up256(n * sizeof(JImg)), o_hf = o_q + up256(quals.size() * sizeof(JQual)), o_coef = o_hf + up256(sizeof(JHuff)),
                 o_dc = o_coef + up256(nb * 128), o_acb = o_dc + up256(nb * 4), o_off = o_acb + up256(nb * 4), o_t = o_off + up256(nb * 8),
                 o_cnt = o_t + up256((size_t)n * 8), o_len = o_cnt + up256((size_t)n * G * 4), o_raw = o_len + up256((size_t)n * 8),
                 total = o_raw + up256(rw * 4 + 16);
    const size_t h_up = o_coef, h_len = up256(h_up);
    static thread_local PerDevice<DeviceScratch> scratch_pd;
    static thread_local PerDevice<PinnedScratch> pinned_pd;
    uint8_t* d = (uint8_t*)scratch_pd.cur().get(total, stream);
    uint8_t* h = pinned_pd.cur().get(h_len + (size_t)n * 8, stream);
    if (!d || !h) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg_encode: scratch allocation of %zu bytes failed", total);
    memcpy(h + o_img, imgs.data(), n * sizeof(JImg));
    memcpy(h + o_q, quals.data(), quals.size() * sizeof(JQual));
    memcpy(h + o_hf, &jhuff(), sizeof(JHuff));
    GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, h_up, hipMemcpyHostToDevice, stream));
    const JImg* dimg = (const JImg*)(d + o_img); const JQual* dq = (const JQual*)(d + o_q); const JHuff* dhf = (const JHuff*)(d + o_hf);
    int16_t* coef = (int16_t*)(d + o_coef); int32_t* dc = (int32_t*)(d + o_dc); uint32_t* acb = (uint32_t*)(d + o_acb);
    uint64_t* off = (uint64_t*)(d + o_off); uint64_t* tb = (uint64_t*)(d + o_t); uint32_t* cnt = (uint32_t*)(d + o_cnt);
    int64_t* len = (int64_t*)(d + o_len); uint32_t* raw = (uint32_t*)(d + o_raw);
    const uint32_t NB = (uint32_t)nb, groups = (NB + kWaves - 1) / kWaves, grid = std::min(groups, 1u << 20);
    hipLaunchKernelGGL(k_jenc_fdct, dim3(grid), dim3(64 * kWaves), 0, stream, dimg, n, NB, dq, dhf, coef, dc, acb);
    hipLaunchKernelGGL(k_jenc_scan, dim3(n), dim3(kScanThreads), 0, stream, dimg, dhf, (const int32_t*)dc, (const uint32_t*)acb, off, tb, raw);
    hipLaunchKernelGGL(k_jenc_emit, dim3(grid), dim3(64 * kWaves), 0, stream, dimg, n, NB, dhf, (const int16_t*)coef, (const int32_t*)dc,
                       (const uint64_t*)off, (const uint64_t*)tb, raw);
    hipLaunchKernelGGL(k_jenc_count, dim3(G, n), dim3(kStuffThreads), 0, stream, dimg, (const uint64_t*)tb, (const uint32_t*)raw, cnt);
    hipLaunchKernelGGL(k_jenc_stuff, dim3(G, n), dim3(kStuffThreads), 0, stream, dimg, dq, (const uint64_t*)tb, (const uint32_t*)raw,
                       (const uint32_t*)cnt, out, len);
    if (int rc = launch_status("jpeg_encode")) return rc;
    int64_t* hlen = (int64_t*)(h + h_len);
    GAMUT_HIP_CHECK(hipMemcpyAsync(hlen, len, (size_t)n * 8, hipMemcpyDeviceToHost, stream));
    GAMUT_HIP_CHECK(hipStreamSynchronize(stream));
    for (int k = 0; k < n; ++k) out_len[which[(size_t)k]] = hlen[k];
    return GAMUT_HIP_OK;
}

int jencode_batch(const uint8_t* const* src, const int64_t* src_pitch, const int32_t* width, const int32_t* height, const int32_t* comp,
                  const int32_t* quality, int count, const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host,
                  hipStream_t stream)
{
    std::vector<JQual> quals; std::vector<int> qkey;                   // key: scale * 2 + sub
    std::vector<JImg> imgs; std::vector<int> which;
    int first_bad = -1;
    for (int i = 0; i < count; ++i) {
        out_len[i] = 0;
        const bool ok = jvalid(width[i], height[i], comp[i]) && src[i] && out_offset[i] >= 0;
        if (status_host) status_host[i] = ok ? GAMUT_HIP_OK : GAMUT_HIP_ERR_INVALID_ARG;
        if (!ok) { if (first_bad < 0) first_bad = i; continue; }
        int scale, sub; jquality(quality ? quality[i] : 90, scale, sub);
        const int key = scale * 2 + sub;
        int qi = (int)(std::find(qkey.begin(), qkey.end(), key) - qkey.begin());
        if (qi == (int)qkey.size()) { qkey.push_back(key); quals.emplace_back(); jqual_build(quals.back(), scale, sub); }
        JImg im{};
        im.src = src[i]; im.pitch = src_pitch[i]; im.out_off = out_offset[i];
        im.w = (uint32_t)width[i]; im.h = (uint32_t)height[i]; im.comp = (uint32_t)comp[i]; im.sub = (uint32_t)sub; im.q = (uint32_t)qi;
        im.mcux = sub ? (im.w + 15) / 16 : (im.w + 7) / 8;
        im.nblk = (uint32_t)jblocks(width[i], height[i], sub);
        imgs.push_back(im); which.push_back(i);
    }
    // chunks of consecutive valid images, at most kChunkBlocks blocks each (an image larger than that goes alone)
    size_t a = 0;
    while (a < imgs.size()) {
        size_t b = a; uint64_t nb = 0;
        while (b < imgs.size() && b - a < kChunkImages && (b == a || nb + imgs[b].nblk <= kChunkBlocks)) nb += imgs[b++].nblk;
        std::vector<JImg> part(imgs.begin() + a, imgs.begin() + b);
        std::vector<int> w(which.begin() + a, which.begin() + b);
        if (int rc = jencode_chunk(part, quals, w, out_len, out, stream)) return rc;
        a = b;
    }
    if (first_bad >= 0) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "image %d: jpeg_encode: invalid size, comp or source", first_bad);
    return GAMUT_HIP_OK;
}

} // namespace
} // namespace gamut

using namespace gamut;

extern "C" {

int64_t gamut_hip_jpeg_encode_bound(int width, int height, int comp, int quality) { return jbound(width, height, comp, quality); }

int gamut_hip_jpeg_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const int32_t* width, const int32_t* height,
                                       const int32_t* comp, const int32_t* quality, int count, const int64_t* out_offset, uint8_t* out,
                                       int64_t* out_len, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!src || !src_pitch || !width || !height || !comp || !out_offset || !out || !out_len)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "jpeg_encode_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return jencode_batch(src, src_pitch, width, height, comp, quality, count, out_offset, out, out_len, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg_encode_batch_device: out of host memory");
    }
}

// host pixels up through pinned staging (rows packed), one image through the batch path; malloc'd stream or NULL
void* gamut_hip_jpeg_encode(const void* data, int width, int height, int comp, int pitch, int quality, int* out_len)
{
    clear_error();
    if (!data || !out_len || !jvalid(width, height, comp)) { set_error(GAMUT_HIP_ERR_INVALID_ARG, "jpeg_encode: invalid arguments"); return nullptr; }
    if (!have_device()) return nullptr;
    const int32_t w = width, hh = height, c = comp, q = quality;
    return encode_host_image("jpeg_encode", HostRows{ data, pitch, (size_t)width * comp, height, 1, 0 }, (size_t)jbound(width, height, comp, quality), out_len,
        [&](const uint8_t* src, int64_t p, int64_t, int64_t off, uint8_t* d, int64_t* len, hipStream_t st) {
            int status = 0;
            return jencode_batch(&src, &p, &w, &hh, &c, &q, 1, &off, d, len, &status, st);
        });
}

// drop-in for stbi_write_jpg_to_func: the whole stream in one call of func
int gamut_hip_jpeg_write_to_func(gamut_hip_jpeg_write_func func, void* context, int x, int y, int comp, const void* data, int pitch, int quality)
{
    if (!func) { clear_error(); set_error(GAMUT_HIP_ERR_INVALID_ARG, "jpeg_write_to_func: no write function"); return 0; }
    int n = 0;
    void* p = gamut_hip_jpeg_encode(data, x, y, comp, pitch, quality, &n);
    if (!p) return 0;
    func(context, p, n);
    free(p);
    return 1;
}

} // extern "C"
