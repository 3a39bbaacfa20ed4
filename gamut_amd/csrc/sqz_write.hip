// sqz_write.hip -- the SQZ back half on the GPU: the reference's coefficient buffer in HBM (as sqz_encode.hip's front half leaves it) ->
// the file SQZ_encode_header and SQZ_schedule_task (source/gamut/codecs/sqz.d:1866-2168) write, bit for bit, cut at the byte budget.
// The serial restatement is sqz_host.hip's Encoder; this file computes the same bits without its lists.
//
// WHY THE STREAM IS DATA-PARALLEL.  Take a band's coefficients v[k] in scan order (its initial LIP) and its max_bitplane m (0..14, from
// the maximum compared as SHORTS).  The class s[k] is the highest bit position in 1..m that is set in v[k], 0 if none; bit 15 is never
// looked at (the reference is blind to it), bit 0 is the sign.  The band is visited at planes p = m .. 1 (once, for its header nibble
// alone, when m is 0).
//   sorting pass at p: the LIP then is {k : s[k] <= p} in scan order; the elements of class p are emitted in scan order, each as
//     [1 unless it is the first] [sign] [WDR code of run], run = 1 + the number of elements of a class BELOW p since the last element
//     of class p (since the band's start for the first); the pass ends with [1] [1 if anything was emitted] [code of 1 + the elements
//     below p behind the last one] [1].  It is skipped when the LIP is empty.  The code of a run is the run's bits under its top
//     bit, each behind a 0: 2 * (ilog2(run) - 1) bits (the reference writes it in two parts above 32 bits; the bits are the same).
//   refinement pass at p: bit p of every element of a class above p, in LSP order: class descending, then scan order.  An element's
//     place in that order does not depend on p: one permutation per band.
// SQZ_schedule_task's order of the (band, plane) visits depends on the bands' m alone, and the writer never looks back: the file is
// the first 8 * budget bits of header + segments in that order, len = (min(bits, 8 * budget) + 7) / 8.
//
// LAUNCHES: SIX per chunk of images, whatever the chunk holds (a chunk is as many images as have 2^29 coefficients between them, at
// most 4096; one image above that is a chunk of its own).  An image takes 96 band slots ([plane 3][level 8][orientation 4]).
//   1. k_sqzw_gather : every band into scan order as compact 16-bit values (through the band's (x, y) table; raster needs none),
//                      and the band's maximum as a short (atomicMax of per-wave maxima).
//   2. k_sqzw_sort<0>: ONE WAVE per band walks it in steps of kChunk = 512 coefficients (eight loads per lane in flight), 64 at a
//                      time: two ballots per class present among the 64 give every lane its run and cost, seven more (one per
//                      bit of the cost) the bit offsets inside each class.  What is carried from step to step -- per class the
//                      count, the elements below it since its last element, the sorting bits so far -- lives in lane `class` of
//                      the wave.  Leaves those three per band and class.
//   3. k_sqzw_walk   : one lane per image: SQZ_schedule_task over the 96 slots (at most 75 bands x 15 visits), the bit offset of
//                      every header nibble, sorting and refinement segment that begins before the cut, the total, deviation (1).
//      -- the call waits here and reads 16 bytes per image: the total bits (which size the file scratch) and the refusal flag --
//   4. k_sqzw_sort<1>: pass 2 again, now writing each element's bits at its offset (atomicOr into the zeroed file scratch, at most
//                      64 bits per element, cut at the budget), the terminations, the header and the nibbles, and scattering the
//                      values into LSP order.  Bands the schedule never reached are skipped whole.
//   5. k_sqzw_refine : per (band, plane) that begins before the cut: one thread per 32-bit word of the file gathers bit p of 32
//                      values in LSP order; only a segment's first and last word need the atomic.  Cut at the budget.
//   6. k_sqzw_place  : the files from scratch to out + out_offset[i], byte by byte: nothing outside [offset, offset + len) is written.
//      (when the files go to the host, 6 is one download of the file scratch instead)
// plus three memsets (the maxima, the file scratch -- cleared on EVERY call: the bits are ORed in) and the small table copies.
// NOTHING proportional to pixels crosses the bus: up go 40 bytes per band slot, down come 16 bytes per image.
//
// SCRATCH per chunk: 2 + 2 bytes per coefficient (compact values, LSP order), 0.9 KB per band slot, and the files: at most
// min(budget, bits used) + 20 bytes each -- with 2^29 coefficients a chunk takes 2 GiB plus its files.  The (x, y) tables are kept per
// thread and device, one per distinct (order, band width, band height), 4 bytes per coefficient of the band; when they pass 1 GiB
// the next call drops them all and builds what it needs.
//
// LIMITS.  A band holds at most 32768 * 32768 = 2^30 coefficients (sides are at most 65535), so counts, runs and indices inside a
// band fit 32 bits; everything with a band, plane or image offset in it -- compact positions, bit offsets, segment lengths, file
// offsets -- is 64 bits.  No geometry SQZ admits is out of the kernels' reach; what cannot be allocated is GAMUT_HIP_ERR_OUT_OF_MEMORY.
// A budget above 2^56 bytes counts as 2^56 (8 * budget must fit 64 bits).
#include "sqz_write.hpp"
#include <climits>

namespace gamut {
namespace {

constexpr int kChunk = 512;                                         // coefficients per step of a wave's walk over its band
constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr uint64_t kNone = ~0ull;
constexpr uint64_t kChunkCoeffs = 1ull << 29;
constexpr size_t kChunkImages = 4096;
constexpr int kGatherY = 32, kPlaceX = 64;

struct WBand { const uint32_t* table; int64_t coeff_base; uint64_t comp_base; uint32_t n, bw, stride; int32_t round; };     // n == 0: an empty slot
struct WImg { uint64_t limit, hdr48; };                             // 8 * budget; the 48 header bits
struct WStat { uint32_t cnt[16], gap[16]; uint64_t bits[16]; };     // per band and class, from pass 2
struct WSeg { uint64_t hdr, sort[16], ref[16]; uint32_t refn[16]; };   // bit offsets in the file (kNone: not emitted); refn: LSP elements refined at p
struct WRes { uint64_t bits; int32_t refused, pad; };

__device__ __forceinline__ uint32_t rl32(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
__device__ __forceinline__ uint64_t rl64(uint64_t v, int lane) { return ((uint64_t)rl32((uint32_t)(v >> 32), lane) << 32) | rl32((uint32_t)v, lane); }
__device__ __forceinline__ int top_bit(uint32_t x) { return 31 - __clz((int)x); }                    // x > 0
__device__ __forceinline__ int max_bitplane(int mx) { const uint32_t h = (uint32_t)(mx >> 1); return h ? top_bit(h) + 1 : 0; }   // SQZ_ilog2(max >> 1)
__device__ __forceinline__ uint64_t interleave64(uint32_t run)     // SQZ_interleave :548-556 on both halves of the run at once
{
    uint64_t x = run;
    x = (x | (x << 16)) & 0x0000FFFF0000FFFFull; x = (x | (x << 8)) & 0x00FF00FF00FF00FFull; x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x << 2)) & 0x3333333333333333ull; x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}
// [prefix: pbits bits][the WDR code of run] -> the value and its width (at most 2 + 62 bits)
__device__ __forceinline__ uint64_t with_run(uint32_t prefix, int pbits, uint32_t run, int* width)
{
    const int cb = 2 * top_bit(run);
    *width = pbits + cb;
    return ((uint64_t)prefix << cb) | (interleave64(run) & ((1ull << cb) - 1ull));
}
// the low `width` (1..64) bits of `value`, most significant first, at bit `pos` of the file (bit 0 = the top bit of byte 0); what
// lies at or behind `limit` is dropped.  The file is zeroed 32-bit words: the bits are ORed in.
__device__ __forceinline__ void put_bits(uint32_t* file, uint64_t pos, uint64_t value, int width, uint64_t limit)
{
    if (width <= 0 || pos >= limit) return;
    if (pos + (uint64_t)width > limit) { const int drop = (int)(pos + (uint64_t)width - limit); value >>= drop; width -= drop; }
    const uint64_t left = value << (64 - width);
    const uint32_t sh = (uint32_t)pos & 31u;
    const uint64_t w = pos >> 5, rest = left << (32u - sh);
    const uint32_t w0 = (uint32_t)(left >> (32u + sh)), w1 = (uint32_t)(rest >> 32), w2 = (uint32_t)rest;
    if (w0) atomicOr(file + w, __builtin_bswap32(w0));
    if (w1) atomicOr(file + w + 1, __builtin_bswap32(w1));
    if (w2) atomicOr(file + w + 2, __builtin_bswap32(w2));
}

__global__ __launch_bounds__(kThreads) void k_sqzw_gather(const WBand* __restrict__ bands, const int16_t* __restrict__ coeffs,
                                                          uint16_t* __restrict__ comp, int* __restrict__ band_max)
{
    const WBand b = bands[blockIdx.x];
    int mx = INT_MIN;
    for (uint32_t k = blockIdx.y * kThreads + threadIdx.x; k < b.n; k += kGatherY * kThreads) {
        uint32_t x, y;
        if (b.table) { const uint32_t xy = b.table[k]; x = xy & 0xFFFFu; y = xy >> 16; }
        else { y = k / b.bw; x = k - y * b.bw; }
        const int16_t v = coeffs[b.coeff_base + (int64_t)y * b.stride + x];
        comp[b.comp_base + k] = (uint16_t)v;
        mx = max(mx, (int)v);
    }
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, __shfl_xor(mx, d, 64));
    if ((threadIdx.x & 63) == 0 && mx != INT_MIN) atomicMax(band_max + blockIdx.x, mx);
}

template <bool EMIT>
__global__ __launch_bounds__(kThreads) void k_sqzw_sort(const WBand* __restrict__ bands, int n_bands, const WImg* __restrict__ imgs,
                                                        const uint16_t* __restrict__ comp, const int* __restrict__ band_max, WStat* __restrict__ stat,
                                                        const WSeg* __restrict__ seg, const uint64_t* __restrict__ file_off, uint32_t* __restrict__ files,
                                                        uint16_t* __restrict__ lsp)
{
    const int lane = threadIdx.x & 63, band = (int)blockIdx.x * kWaves + (int)(threadIdx.x >> 6);
    if (band >= n_bands) return;
    const WBand b = bands[band];
    if (!b.n) return;
    const int mx = band_max[band];
    if (mx < 0) return;                                             // deviation (1): refused if the schedule reaches the band, else not in the file
    const int m = max_bitplane(mx);
    uint32_t* file = nullptr;
    uint64_t limit = 0, soff = kNone;
    uint32_t lbase = 0;                                             // lane c: the elements of a class above c = where class c begins in LSP order
    if (EMIT) {
        const int img = band / kSqzSlots;
        const uint64_t fo = file_off[img];
        const WSeg& sg = seg[band];
        if (fo == kNone || sg.hdr == kNone) return;
        file = files + fo; limit = imgs[img].limit;
        if (lane == 0) {
            if (band % kSqzSlots == 0) put_bits(file, 0, imgs[img].hdr48, 48, limit);
            put_bits(file, sg.hdr, (uint64_t)m, 4, limit);
        }
        if (lane >= 1 && lane <= 14) soff = sg.sort[lane];
        if (lane < 16) for (int c = lane + 1; c <= 14; ++c) lbase += stat[band].cnt[c];
    }
    uint32_t cnt = 0, gap = 0;                                      // lane c: elements of class c so far; elements below c since the last of them
    uint64_t bits = 0;                                              // lane c: the sorting bits of plane c so far
    if (m > 0) {
        const uint32_t vmask = (2u << m) - 1u;
        const uint64_t below = (1ull << lane) - 1ull;
        for (uint32_t k0 = 0; k0 < b.n; k0 += kChunk) {
            uint16_t v[kChunk / 64];
            #pragma unroll
            for (int j = 0; j < kChunk / 64; ++j) {
                const uint32_t idx = k0 + (uint32_t)j * 64u + (uint32_t)lane;
                v[j] = idx < b.n ? comp[b.comp_base + idx] : (uint16_t)0;
            }
            #pragma unroll
            for (int j = 0; j < kChunk / 64; ++j) {
                const uint32_t g0 = k0 + (uint32_t)j * 64u;
                if (g0 >= b.n) break;
                const bool valid = g0 + (uint32_t)lane < b.n;
                const uint32_t r = ((uint32_t)v[j] & vmask) >> 1;
                const int s = valid ? (r ? top_bit(r) + 1 : 0) : 31;            // 31: behind the band's end, neither equal to nor below a class
                const uint64_t vm = __ballot(valid);
                uint64_t todo = __ballot(valid && s > 0);
                if (!todo) {                                        // nothing significant among the 64
                    if (lane >= 1 && lane <= m) gap += (uint32_t)__popcll(vm);
                    continue;
                }
                uint32_t handled = 0;
                // per class present: two ballots, and every lane of the class takes what it needs of the class's state (kept in lane c)
                uint64_t my_eb = 0, my_lt = 0, own_eq = 0, my_so = kNone, my_sofar = 0;
                uint32_t my_cnt = 0, my_gap = 0, my_lb = 0;
                while (todo) {
                    const int c = (int)rl32((uint32_t)s, __ffsll((unsigned long long)todo) - 1);
                    const uint64_t eq = __ballot(s == c), lt = __ballot(s < c);
                    todo &= ~eq; handled |= 1u << c;
                    const uint32_t cnt_c = rl32(cnt, c), gap_c = rl32(gap, c);
                    if (s == c) { my_eb = eq & below; my_lt = lt & below; my_cnt = cnt_c; my_gap = gap_c; }
                    if (EMIT) {
                        const uint64_t so = rl64(soff, c), sofar = rl64(bits, c);
                        const uint32_t lb = rl32(lbase, c);
                        if (s == c) { my_so = so; my_sofar = sofar; my_lb = lb; }
                    }
                    const int last = 63 - __clzll((long long)eq);
                    if (lane == c) { own_eq = eq; cnt += (uint32_t)__popcll(eq); gap = (uint32_t)__popcll(lt & ~((2ull << last) - 1ull)); }
                }
                // once per 64: every significant lane's run and cost, then the costs (at most 64: seven bits) of the lanes of its class
                // below it, and in lane c of the whole class: a ballot per bit
                const bool sig = valid && s > 0;
                uint32_t run = 1; int cost = 0; bool first = false;
                if (sig) {
                    if (my_eb) { const int prev = 63 - __clzll((long long)my_eb); run = 1u + (uint32_t)__popcll(my_lt & ~((2ull << prev) - 1ull)); }
                    else { run = 1u + my_gap + (uint32_t)__popcll(my_lt); first = my_cnt == 0; }
                    cost = (first ? 1 : 2) + 2 * top_bit(run);
                }
                uint32_t before = 0, total = 0;
                #pragma unroll
                for (int bit = 0; bit < 7; ++bit) {
                    const uint64_t mb = __ballot((cost >> bit) & 1);
                    total += (uint32_t)__popcll(mb & own_eq) << bit;
                    if (EMIT) before += (uint32_t)__popcll(mb & my_eb) << bit;
                }
                if (EMIT && sig) {
                    if (my_so != kNone) {
                        int width;
                        const uint64_t value = with_run((first ? 0u : 2u) | ((uint32_t)v[j] & 1u), first ? 1 : 2, run, &width);
                        put_bits(file, my_so + my_sofar + before, value, width, limit);
                    }
                    lsp[b.comp_base + my_lb + my_cnt + (uint32_t)__popcll(my_eb)] = v[j];
                }
                bits += total;                                      // (own_eq is 0 in a lane whose class is not among the 64)
                for (int c = 1; c <= m; ++c) {                      // the classes that are not among the 64 count what is below them
                    if (handled >> c & 1u) continue;
                    const uint64_t lt = __ballot(s < c);
                    if (lane == c) gap += (uint32_t)__popcll(lt);
                }
            }
        }
    }
    if (!EMIT) {
        if (lane < 16) { stat[band].cnt[lane] = cnt; stat[band].gap[lane] = gap; stat[band].bits[lane] = bits; }
    } else if (lane >= 1 && lane <= m && soff != kNone && lbase < b.n) {         // the WDR termination of plane `lane` (its LIP is not empty)
        int width;
        const uint64_t value = with_run(cnt ? 3u : 1u, cnt ? 2 : 1, 1u + gap, &width);
        put_bits(file, soff + bits, value, width, limit);
        put_bits(file, soff + bits + (uint64_t)width, 1u, 1, limit);
    }
}

// SQZ_schedule_task :2105-2168 (sqz_host.hip: Coder::walk) for image blockIdx.x * 64 + threadIdx.x, on lengths in place of a bit writer
__global__ __launch_bounds__(64) void k_sqzw_walk(const WBand* __restrict__ bands, const WImg* __restrict__ imgs, int n_img, const int* __restrict__ band_max,
                                                  const WStat* __restrict__ stat, WSeg* __restrict__ seg, WRes* __restrict__ res, const uint8_t* __restrict__ shape)
{
    const int i = (int)(blockIdx.x * 64u + threadIdx.x);
    if (i >= n_img) return;
    const int base = i * kSqzSlots;
    const uint64_t limit = imgs[i].limit;
    const uint32_t planes = shape[2 * i], levels = shape[2 * i + 1];
    int8_t bp[kSqzSlots];
    for (int s = 0; s < kSqzSlots; ++s) {
        WSeg& sg = seg[base + s];
        sg.hdr = kNone;
        for (int c = 0; c < 16; ++c) { sg.sort[c] = kNone; sg.ref[c] = kNone; sg.refn[c] = 0; }
        bp[s] = 0;
    }
    uint64_t off = 48;
    int refused = 0;
    uint32_t state = 0, plane = 0, level = 0, o = 0;
    int round = 0; bool done = false, stop = false;
    while (!done && off < limit && !stop) {
        done = true;
        for (;;) {
            const int slot = (int)((plane * kSqzLevels + level) * kSqzOrients + o), g = base + slot;
            const int br = bands[g].round;
            if (round < br || (round > br && bp[slot] == 0)) done = done && round > br;
            else {
                WSeg& sg = seg[g];
                if (br == round) {                                  // SQZ_encode_init_subband
                    const int mx = band_max[g];
                    if (mx < 0) { refused = 1; stop = true; break; }
                    bp[slot] = (int8_t)max_bitplane(mx);
                    sg.hdr = off; off += 4;
                }
                const int p = bp[slot];
                if (p > 0 && off < limit) {
                    const WStat& st = stat[g];
                    uint32_t above = 0;
                    for (int c = p + 1; c <= 14; ++c) above += st.cnt[c];
                    if (above < bands[g].n) {                       // the sorting pass: the LIP is not empty
                        sg.sort[p] = off;
                        off += st.bits[p] + (st.cnt[p] ? 2u : 1u) + 2u * (uint32_t)top_bit(1u + st.gap[p]) + 1u;
                    }
                    if (above && off < limit) { sg.ref[p] = off; sg.refn[p] = above; off += above; }
                }
                bp[slot] -= p > 0;
                if (off >= limit) { stop = true; break; }
                done = done && bp[slot] == 0;
            }
            if (!state) {                                           // plane 0 alone
                if (++o >= (uint32_t)kSqzOrients) {
                    ++level;
                    o = level < levels;
                    if (o == 0u) { level = 0; state = plane = planes > 1u; if (!state) break; }
                }
            } else if (++plane >= planes) {                         // planes 1.. per orientation
                plane = 1;
                if (++o >= (uint32_t)kSqzOrients) {
                    ++level;
                    o = level < levels;
                    if (o == 0u) { level = 0; state = plane = 0; break; }
                }
            }
        }
        ++round;
    }
    res[i].bits = off < limit ? off : limit;
    res[i].refused = refused;
    res[i].pad = 0;
}

__global__ __launch_bounds__(kThreads) void k_sqzw_refine(const WBand* __restrict__ bands, const WImg* __restrict__ imgs, const WSeg* __restrict__ seg,
                                                          const uint64_t* __restrict__ file_off, uint32_t* __restrict__ files, const uint16_t* __restrict__ lsp)
{
    const int band = (int)blockIdx.x, p = (int)blockIdx.y + 1, img = band / kSqzSlots;
    const uint64_t off = seg[band].ref[p], fo = file_off[img];
    if (off == kNone || fo == kNone) return;
    const uint64_t limit = imgs[img].limit;                         // off < limit: the walk only records segments that begin before the cut
    const uint64_t n = min((uint64_t)seg[band].refn[p], limit - off);
    uint32_t* file = files + fo;
    const uint16_t* src = lsp + bands[band].comp_base;
    const uint64_t w0 = off >> 5, w1 = (off + n - 1) >> 5;
    for (uint64_t w = w0 + threadIdx.x; w <= w1; w += kThreads) {
        const int64_t e0 = (int64_t)(w << 5) - (int64_t)off;        // the element whose bit is the word's first
        uint32_t word = 0;
        #pragma unroll 8
        for (int j = 0; j < 32; ++j) {
            const int64_t e = e0 + j;
            if (e >= 0 && (uint64_t)e < n) word |= (((uint32_t)src[e] >> p) & 1u) << (31 - j);
        }
        if (!word) continue;
        if (w == w0 || w == w1) atomicOr(file + w, __builtin_bswap32(word));
        else file[w] = __builtin_bswap32(word);                     // wholly inside the segment: nobody else writes it
    }
}

__global__ __launch_bounds__(kThreads) void k_sqzw_place(const uint64_t* __restrict__ file_off, const int64_t* __restrict__ out_off, const int64_t* __restrict__ lens,
                                                         const uint32_t* __restrict__ files, uint8_t* __restrict__ out)
{
    const uint64_t fo = file_off[blockIdx.y];
    if (fo == kNone) return;
    const uint8_t* src = reinterpret_cast<const uint8_t*>(files + fo);
    uint8_t* dst = out + out_off[blockIdx.y];
    const int64_t n = lens[blockIdx.y];
    for (int64_t k = (int64_t)blockIdx.x * kThreads + threadIdx.x; k < n; k += (int64_t)kPlaceX * kThreads) dst[k] = src[k];
}

thread_local float t_write_ms[2] = { -1.0f, -1.0f };

// the calling thread's writer state on one device
struct Writer {
    DeviceScratch blob, comp, lsp, files;
    PinnedScratch pinned, staged;
};

struct Job {
    const int16_t* coeffs; const int64_t* coeff_offset; const gamut_hip_sqz_encode_desc* descs; const int* which;
    const int64_t* out_offset; uint8_t* out; bool out_on_device; int64_t* out_len; int* rcs; hipStream_t stream; bool timing;
};

int write_chunk(Writer& W, SqzScanTables& T, const Job& J, size_t a, size_t b)
{
    const size_t n = b - a, nb = n * kSqzSlots;
    hipStream_t stream = J.stream;
    // ---- the tables: bands, images, and what the kernels leave
    const size_t o_bands = 0, o_imgs = o_bands + up256(nb * sizeof(WBand)), o_shape = o_imgs + up256(n * sizeof(WImg)), up_bytes = o_shape + up256(2 * n);
    const size_t o_max = up_bytes, o_stat = o_max + up256(nb * sizeof(int)), o_seg = o_stat + up256(nb * sizeof(WStat)), o_res = o_seg + up256(nb * sizeof(WSeg));
    const size_t o_foff = o_res + up256(n * sizeof(WRes)), o_ooff = o_foff + up256(n * 8), o_lens = o_ooff + up256(n * 8), total = o_lens + up256(n * 8);
    const size_t h_res = up_bytes, h_foff = h_res + up256(n * sizeof(WRes)), h_total = h_foff + 3 * up256(n * 8);
    uint8_t* d = (uint8_t*)W.blob.get(total, stream);
    uint8_t* h = W.pinned.get(h_total, stream);
    if (!d || !h) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_write: %zu bytes of tables could not be had", total);
    memset(h, 0, up_bytes);
    WBand* hb = (WBand*)(h + o_bands); WImg* hi = (WImg*)(h + o_imgs); uint8_t* hs = h + o_shape;
    uint64_t elems = 0;
    const TracePoint t_tab = trace_now();
    for (size_t k = 0; k < n; ++k) {
        const int i = J.which[a + k];
        const gamut_hip_sqz_encode_desc& D = J.descs[i];
        SqzBandGeom g[kSqzSlots];
        sqz_band_geometry(D, g);
        for (int s = 0; s < kSqzSlots; ++s) {
            WBand& B = hb[k * kSqzSlots + (size_t)s];
            B.round = g[s].round;
            if (!g[s].width) continue;
            B.n = g[s].width * g[s].height; B.bw = g[s].width; B.stride = g[s].stride;
            B.coeff_base = J.coeff_offset[i] + g[s].offset; B.comp_base = elems;
            elems += B.n;
            if (D.scan_order != 0 && !(B.table = T.table(D.scan_order, g[s].width, g[s].height))) return GAMUT_HIP_ERR_OUT_OF_MEMORY;
        }
        const uint64_t budget = (uint64_t)std::min<int64_t>(D.budget, (int64_t)1 << 56);
        hi[k].limit = budget * 8u;
        hi[k].hdr48 = (0xA5ull << 40) | ((uint64_t)(D.width - 1) << 24) | ((uint64_t)(D.height - 1) << 8) | ((uint64_t)D.color_mode << 6) |
                      ((uint64_t)(D.levels - 1) << 3) | ((uint64_t)D.scan_order << 1) | (uint64_t)(D.subsampling != 0);
        hs[2 * k] = D.color_mode == 0 ? 1 : 3; hs[2 * k + 1] = (uint8_t)D.levels;
    }
    if (J.timing) t_write_ms[1] += (float)ms_since(t_tab);
    uint16_t* comp = (uint16_t*)W.comp.get((size_t)(elems + 8) * 2, stream);
    uint16_t* lsp = (uint16_t*)W.lsp.get((size_t)(elems + 8) * 2, stream);
    if (!comp || !lsp) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_write: %llu bytes of band scratch could not be had", (unsigned long long)elems * 4);
    const WBand* dbands = (const WBand*)(d + o_bands); const WImg* dimgs = (const WImg*)(d + o_imgs);
    int* dmax = (int*)(d + o_max); WStat* dstat = (WStat*)(d + o_stat); WSeg* dseg = (WSeg*)(d + o_seg); WRes* dres = (WRes*)(d + o_res);
    uint64_t* dfoff = (uint64_t*)(d + o_foff); int64_t* dooff = (int64_t*)(d + o_ooff); int64_t* dlens = (int64_t*)(d + o_lens);
    StreamDrain drain;
    GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, up_bytes, hipMemcpyHostToDevice, stream));
    drain.arm(stream);
    GAMUT_HIP_CHECK(hipMemsetAsync(dmax, 0x80, nb * sizeof(int), stream));      // 0x80808080: below every short
    float ms[2] = { 0, 0 };
    {
        KernelTimer<2> timer(J.timing);
        timer.mark(stream);
        hipLaunchKernelGGL(k_sqzw_gather, dim3((unsigned)nb, kGatherY), dim3(kThreads), 0, stream, dbands, J.coeffs, comp, dmax);
        hipLaunchKernelGGL(k_sqzw_sort<false>, dim3((unsigned)((nb + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream, dbands, (int)nb, dimgs, (const uint16_t*)comp,
                           (const int*)dmax, dstat, (const WSeg*)dseg, (const uint64_t*)dfoff, (uint32_t*)nullptr, lsp);
        hipLaunchKernelGGL(k_sqzw_walk, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, dbands, dimgs, (int)n, (const int*)dmax, (const WStat*)dstat, dseg, dres,
                           (const uint8_t*)(d + o_shape));
        if (int rc = launch_status("sqz_write")) return rc;
        timer.mark(stream);
        GAMUT_HIP_CHECK(hipMemcpyAsync(h + h_res, dres, n * sizeof(WRes), hipMemcpyDeviceToHost, stream));
        const hipError_t e = drain.wait();
        if (e != hipSuccess) return set_error(GAMUT_HIP_ERR_HIP, "sqz_write: %s", hipGetErrorString(e));
        timer.finish(&ms[0]);
    }
    // ---- the totals size the files; a refused image has none
    const WRes* hres = (const WRes*)(h + h_res);
    uint64_t* hfoff = (uint64_t*)(h + h_foff); int64_t* hooff = (int64_t*)(h + h_foff + up256(n * 8)); int64_t* hlens = (int64_t*)(h + h_foff + 2 * up256(n * 8));
    uint64_t words = 0;
    for (size_t k = 0; k < n; ++k) {
        const int i = J.which[a + k];
        hooff[k] = J.out_offset[i];
        if (hres[k].refused) { J.rcs[a + k] = sqz_undefined_shift_error(); hfoff[k] = kNone; hlens[k] = 0; J.out_len[i] = 0; continue; }
        hlens[k] = (int64_t)((hres[k].bits + 7u) / 8u);
        hfoff[k] = words;
        words += ((uint64_t)hlens[k] + 3u) / 4u + 4u;
        J.out_len[i] = hlens[k];
    }
    uint32_t* files = (uint32_t*)W.files.get((size_t)words * 4 + 16, stream);
    if (!files) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_write: %llu bytes of file scratch could not be had", (unsigned long long)words * 4);
    uint8_t* staged = nullptr;
    if (!J.out_on_device && !(staged = W.staged.get((size_t)words * 4 + 16, stream)))
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_write: %llu bytes of pinned staging could not be had", (unsigned long long)words * 4);
    GAMUT_HIP_CHECK(hipMemcpyAsync(dfoff, hfoff, 3 * up256(n * 8), hipMemcpyHostToDevice, stream));      // file_off, out_off, lens lie 256-aligned one behind another on both sides
    drain.arm(stream);
    GAMUT_HIP_CHECK(hipMemsetAsync(files, 0, (size_t)words * 4 + 16, stream));
    {
        KernelTimer<2> timer(J.timing);
        timer.mark(stream);
        hipLaunchKernelGGL(k_sqzw_sort<true>, dim3((unsigned)((nb + kWaves - 1) / kWaves)), dim3(kThreads), 0, stream, dbands, (int)nb, dimgs, (const uint16_t*)comp,
                           (const int*)dmax, dstat, (const WSeg*)dseg, (const uint64_t*)dfoff, files, lsp);
        hipLaunchKernelGGL(k_sqzw_refine, dim3((unsigned)nb, 14), dim3(kThreads), 0, stream, dbands, dimgs, (const WSeg*)dseg, (const uint64_t*)dfoff, files, (const uint16_t*)lsp);
        if (J.out_on_device)
            hipLaunchKernelGGL(k_sqzw_place, dim3(kPlaceX, (unsigned)n), dim3(kThreads), 0, stream, (const uint64_t*)dfoff, (const int64_t*)dooff, (const int64_t*)dlens,
                               (const uint32_t*)files, J.out);
        if (int rc = launch_status("sqz_write")) return rc;
        timer.mark(stream);
        if (!J.out_on_device && words) GAMUT_HIP_CHECK(hipMemcpyAsync(staged, files, (size_t)words * 4, hipMemcpyDeviceToHost, stream));
        const hipError_t e = drain.wait();
        if (e != hipSuccess) return set_error(GAMUT_HIP_ERR_HIP, "sqz_write: %s", hipGetErrorString(e));
        timer.finish(&ms[1]);
    }
    if (!J.out_on_device)
        for (size_t k = 0; k < n; ++k)
            if (hfoff[k] != kNone) memcpy(J.out + hooff[k], staged + hfoff[k] * 4, (size_t)hlens[k]);
    if (J.timing) t_write_ms[0] = ms[0] < 0 || ms[1] < 0 || t_write_ms[0] < 0 ? -1.0f : t_write_ms[0] + ms[0] + ms[1];
    return GAMUT_HIP_OK;
}

} // namespace

void SqzScanTables::drop_tables()
{
    for (auto& t : tables) (void)hipFree(t.second);
    tables.clear(); table_bytes = 0;
}
const uint32_t* SqzScanTables::table(int order, uint32_t w, uint32_t h)
{
    const auto key = std::make_tuple(order, w, h);
    const auto it = tables.find(key);
    if (it != tables.end()) return it->second;
    const size_t n = (size_t)w * h;
    std::vector<uint32_t> xy(n);                                    // an (x, y) pair of uint16 is x | y << 16
    if (sqz_scan_order(order, (int)w, (int)h, reinterpret_cast<uint16_t*>(xy.data())) != GAMUT_HIP_OK) return nullptr;
    uint32_t* d = nullptr;
    if (hipMalloc((void**)&d, n * 4) != hipSuccess || hipMemcpy(d, xy.data(), n * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        if (d) (void)hipFree(d);
        set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz: a scan table of %zu bytes could not be had", n * 4);
        return nullptr;
    }
    tables[key] = d; table_bytes += n * 4;
    return d;
}
SqzScanTables& sqz_scan_tables()
{
    static thread_local PerDevice<SqzScanTables> pd;
    return pd.cur();
}

int sqz_write_files(const int16_t* coeffs, const int64_t* coeff_offset, const gamut_hip_sqz_encode_desc* descs, const std::vector<int>& which,
                    const int64_t* out_offset, uint8_t* out, bool out_on_device, int64_t* out_len, std::vector<int>& rcs, hipStream_t stream)
{
    static const bool timing = env_flag("GAMUT_HIP_SQZ_TIMING");
    static thread_local PerDevice<Writer> writer_pd;
    rcs.assign(which.size(), GAMUT_HIP_OK);
    if (which.empty()) return GAMUT_HIP_OK;
    Writer& W = writer_pd.cur();
    SqzScanTables& T = sqz_scan_tables();
    if (T.table_bytes > kSqzTableCap) T.drop_tables();                 // (every call ends with a wait on its stream: nothing reads them now)
    if (timing) t_write_ms[0] = t_write_ms[1] = 0.0f;
    const Job J{ coeffs, coeff_offset, descs, which.data(), out_offset, out, out_on_device, out_len, rcs.data(), stream, timing };
    for (size_t a = 0; a < which.size(); ) {
        size_t b = a; uint64_t elems = 0;
        while (b < which.size() && b - a < kChunkImages) {
            const gamut_hip_sqz_encode_desc& D = descs[which[b]];
            const uint64_t e = (uint64_t)D.width * (uint64_t)D.height * (D.color_mode == 0 ? 1u : 3u);
            if (b > a && elems + e > kChunkCoeffs) break;
            elems += e; ++b;
        }
        if (int rc = write_chunk(W, T, J, a, b)) return rc;
        a = b;
    }
    return GAMUT_HIP_OK;
}

} // namespace gamut

using namespace gamut;

extern "C" {

int gamut_hip_sqz_write_batch_device(const int16_t* coeffs, const int64_t* coeff_offset, const gamut_hip_sqz_encode_desc* descs, int count,
                                     const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!coeffs || !coeff_offset || !descs || !out_offset || !out || !out_len)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_write_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        std::vector<gamut_hip_sqz_encode_desc> checked(descs, descs + count);
        std::vector<int> which, rcs;
        SqzRefusals bad; bad.status = status_host;
        for (int i = 0; i < count; ++i) {
            if (status_host) status_host[i] = GAMUT_HIP_OK;
            out_len[i] = 0;
            gamut_hip_sqz_encode_desc& d = checked[(size_t)i];
            int rc = sqz_encode_check(&d);
            if (rc == GAMUT_HIP_OK && d.budget <= 6) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: a budget of %lld bytes does not hold the 6-byte header and one more bit", (long long)d.budget);
            if (rc == GAMUT_HIP_OK && out_offset[i] < 0) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: negative out_offset");
            if (rc == GAMUT_HIP_OK && coeff_offset[i] < 0) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: negative coeff_offset");
            if (rc != GAMUT_HIP_OK) { bad.refuse(i, rc); continue; }
            which.push_back(i);
        }
        if (int rc = sqz_write_files(coeffs, coeff_offset, checked.data(), which, out_offset, out, true, out_len, rcs, pick_stream(stream))) return rc;
        for (size_t k = 0; k < which.size(); ++k)
            if (rcs[k] != GAMUT_HIP_OK) { sqz_undefined_shift_error(); bad.refuse(which[k], rcs[k]); }
        return bad.verdict();
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_write_batch_device: out of host memory");
    }
}

int gamut_hip_sqz_write_chunk(void) { return kChunk; }

float gamut_hip_sqz_last_write_stage_ms(int stage) { return stage >= 0 && stage < 2 ? t_write_ms[stage] : -1.0f; }

} // extern "C"
