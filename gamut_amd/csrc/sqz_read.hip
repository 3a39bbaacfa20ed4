// sqz_read.hip -- the SQZ front end on the GPU: files -> the reference's coefficient buffer in HBM as it stands behind
// SQZ_decode_round_coefficients (source/gamut/codecs/sqz.d:1941-2168), value for value what sqz_host.hip's Decoder writes, ready for
// gamut_hip_sqz_reconstruct_batch_device.  The serial restatement is sqz_host.hip; the rules by bit position are in sqz_read.hpp.
//
// WHAT IS SERIAL AND WHAT IS NOT.  The chain of (band, bit plane) segments is serial: where a segment ends is known only once it has
// been read.  INSIDE a segment every bit position is classified without its neighbours: in a sorting pass the bits at odd offsets from
// the pass's start are flags, a set flag closes a record, and a record's run is a function of the 64 bits in front of its flag and of
// where the flag before it lies; a refinement pass is one bit per LSP entry.  So ONE WORKGROUP of 1024 lanes per file walks the chain
// (SQZ_schedule_task, uniform over the workgroup, the bands' state in LDS) and spends all its lanes inside each segment; the batch
// supplies the rest of the parallelism (one file per compute unit at a time).
//
// A SORTING PASS runs in windows of kWindow = 32 * 1024 bits, a dword per lane:
//   1. the lane masks its flags by parity (sqzr_flags: the end rule included) and counts them;
//   2. a workgroup scan gives every lane the rank of its first record in the window and the flag that closed the record before it;
//   3. the lane computes its records' advances (sqzr_run, sqzr_advance: at most 16 per lane, the work of each fixed);
//   4. a second scan (64-bit sums, with the carry of the windows before) turns advances into targets t = sum - 1 into the LIP AS IT
//      STOOD WHEN THE PASS BEGAN; the targets rise strictly, so "t < |LIP|" alone says whether a record is applied, and the first
//      record that fails it -- found by a minimum over the workgroup -- ends the pass behind its flag;
//   5. applied records set their coefficient's bit and sign (through the list entry, an x | y << 16 pair), append the entry to the
//      band's LSP array behind what is merged, and mark the LIP entry as taken.
// A window without an overshoot hands three carries to the next: the sum, the records so far, the last flag.  A record may span any
// number of windows: nothing is done for it before its flag.  No loop's trip count depends on a run: work is bounded by the bits
// present and the band sizes.
// THE LIP is an array of entries in scan order.  Until a pass takes something from it, it IS the band's scan table (or the raster
// formula) and nothing is stored: a visit that takes nothing costs its windows alone.  The first take materialises it; a pass that
// took something and is followed by more decoding compacts it in place (4096 entries per step: read, scan, write below).
// REFINEMENT: one lane per 32 LSP entries, a 2-byte read-modify-write per set bit; LSP entries are distinct coefficients.
// ROUNDING is the tail of the same kernel, over the merged LSP of every band.  A second kernel (k_sqzr_zero) clears the coefficients
// first, as the reference's calloc does.
//
// SCRATCH: 4 + 4 bytes per coefficient (LIP, LSP) for the files of a chunk; a chunk is as many files as stay under
// gamut_hip_sqz_set_read_chunk coefficients (default 2^31: 16 GiB of lists at most; one larger file is a chunk of its own).  The
// files go up through pinned staging, 40 bytes per band slot with them.  The scan tables are the device writer's (sqz_write.hpp).
// VISIBILITY: the lists and the coefficients are global memory written and read by different waves of ONE workgroup, always with a
// __syncthreads() (a workgroup-scope fence and barrier) between a write and a read of the same address.
#include "sqz_write.hpp"
#include "sqz_read.hpp"

namespace gamut {
int sqz_parse_header(const uint8_t* data, size_t len, gamut_hip_sqz_info* info);                 // sqz_host.hip
namespace {

constexpr int kT = 1024, kWaves = kT / 64, kWindow = 32 * kT;
constexpr int kCompact = 4;                                         // LIP entries per lane and compaction step
constexpr int kZeroX = 32, kZeroThreads = 256;
constexpr size_t kChunkFiles = 16384;

struct RBand { const uint32_t* table; int64_t coeff_off; uint64_t list_base; uint32_t n, bw, stride; int32_t round; };     // n == 0: an empty slot
struct RImg { uint64_t file_off, len; int64_t coeff_base; uint64_t coeffs; uint32_t planes, levels; };

struct OpAdd { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; } };
// high half: a count, added; low half: 1 + the window offset of a lane's last flag, 0 for none: the later one wins
struct OpCountLast { __device__ uint64_t operator()(uint64_t a, uint64_t b) const { return ((a >> 32) + (b >> 32)) << 32 | ((uint32_t)b ? (uint32_t)b : (uint32_t)a); } };

// inclusive scan over the workgroup in thread order (0 is the identity of both operators); two barriers
template <class Op> __device__ __forceinline__ uint64_t block_scan(uint64_t v, Op op, uint64_t* excl, uint64_t* total, uint64_t* s_w)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    #pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t t = (uint64_t)__shfl_up((unsigned long long)v, d, 64);
        if (lane >= d) v = op(t, v);
    }
    uint64_t ex = (uint64_t)__shfl_up((unsigned long long)v, 1, 64);
    if (lane == 0) ex = 0;
    if (lane == 63) s_w[wave] = v;
    __syncthreads();
    uint64_t off = 0, tot = 0;
    #pragma unroll
    for (int i = 0; i < kWaves; ++i) { const uint64_t x = s_w[i]; if (i < wave) off = op(off, x); tot = op(tot, x); }
    __syncthreads();
    *excl = op(off, ex); *total = tot;
    return op(off, v);
}

__device__ __forceinline__ int16_t* coef_at(int16_t* coeffs, const RBand& b, uint32_t xy) { return coeffs + b.coeff_off + (int64_t)(xy >> 16) * b.stride + (xy & 0xFFFFu); }
__device__ __forceinline__ uint32_t scan_entry(const RBand& b, uint32_t k) { if (b.table) return b.table[k]; const uint32_t y = k / b.bw; return y << 16 | (k - y * b.bw); }

__global__ __launch_bounds__(kZeroThreads) void k_sqzr_zero(const RImg* __restrict__ imgs, int16_t* __restrict__ coeffs)
{
    const RImg im = imgs[blockIdx.y];
    int16_t* dst = coeffs + im.coeff_base;
    const uint64_t n = im.coeffs, tid = (uint64_t)blockIdx.x * kZeroThreads + threadIdx.x, step = (uint64_t)kZeroX * kZeroThreads;
    uint64_t head = (8u - ((uintptr_t)dst & 7u)) / 2u & 3u;          // elements in front of the first 8-byte boundary
    if (head > n) head = n;
    const uint64_t quads = (n - head) / 4u, tail = head + quads * 4u;
    if (tid < head) dst[tid] = 0;
    uint2* body = reinterpret_cast<uint2*>(dst + head);
    for (uint64_t k = tid; k < quads; k += step) body[k] = make_uint2(0u, 0u);
    if (tid < n - tail) dst[tail + tid] = 0;
}

// One workgroup per file: the whole chain, then the rounding.
__global__ __launch_bounds__(kT) void k_sqzr_walk(const RBand* __restrict__ bands, const RImg* __restrict__ imgs, const uint8_t* __restrict__ files,
                                                  int16_t* __restrict__ coeffs, uint32_t* __restrict__ lip_all, uint32_t* __restrict__ lsp_all)
{
    __shared__ uint64_t s_w[kWaves];
    __shared__ uint32_t s_lipn[kSqzSlots], s_lspn[kSqzSlots];
    __shared__ int8_t s_bp[kSqzSlots], s_max[kSqzSlots];
    __shared__ uint8_t s_mat[kSqzSlots];
    __shared__ uint32_t s_over;
    const uint32_t tid = threadIdx.x;
    const RImg im = imgs[blockIdx.x];
    const RBand* B = bands + (size_t)blockIdx.x * kSqzSlots;
    const uint8_t* file = files + im.file_off;
    const uint64_t len = im.len;
    const int64_t N = (int64_t)(len * 8u);
    if (tid < (uint32_t)kSqzSlots) { s_lipn[tid] = B[tid].n; s_lspn[tid] = 0; s_bp[tid] = 0; s_max[tid] = 0; s_mat[tid] = 0; }
    __syncthreads();

    // SQZ_schedule_task :2105-2168 (sqz_host.hip: Coder::walk); every lane holds the same pos, round, done and stop
    int64_t pos = 48;
    const uint32_t planes = im.planes, levels = im.levels;
    uint32_t state = 0, plane = 0, level = 0, o = 0;
    int round = 0; bool done = false, stop = false;
    while (!done && pos < N && !stop) {
        done = true;
        for (;;) {
            const int slot = (int)((plane * kSqzLevels + level) * kSqzOrients + o);
            const RBand b = B[slot];
            const int bp0 = s_bp[slot];
            if (round < b.round || (round > b.round && bp0 == 0)) done = done && round > b.round;
            else {
                // ---- one visit: SQZ_decode_init_subband on the first, then SQZ_decode_bitplane :2070-2080
                int bp = bp0, mx = s_max[slot];
                if (b.round == round) { mx = bp = sqzr_nibble(file, len, &pos); }
                const uint32_t n = s_lipn[slot], lspn = s_lspn[slot];
                uint32_t* lip = lip_all + b.list_base;
                uint32_t* lsp = lsp_all + b.list_base;
                uint32_t nsp = 0;
                bool go = true, mat = s_mat[slot] != 0;
                if (n != 0u && bp > 0) {                            // the sorting pass :1988-2020
                    const uint32_t mask = 1u << bp;
                    const int64_t s = pos;
                    int64_t carry_prev = s - 1;
                    uint64_t carry_sum = 0;
                    bool closed = false;
                    for (int64_t P = s; P < N; P += kWindow) {
                        const int64_t p = P + 32 * (int64_t)tid;
                        const uint32_t word = p < N ? sqzr_bits32(file, len, p) : 0u;
                        const uint32_t fl = sqzr_flags(word, p, s, N);
                        const uint32_t cnt = (uint32_t)__popc(fl);
                        const uint32_t last = fl ? 32u * tid + (31u - (uint32_t)(__ffs((int)fl) - 1)) + 1u : 0u;
                        uint64_t exA, totA;
                        block_scan((uint64_t)cnt << 32 | last, OpCountLast(), &exA, &totA, s_w);
                        const int64_t pv = (uint32_t)exA ? P + (int64_t)(uint32_t)exA - 1 : carry_prev;
                        uint64_t sum = 0, first_adv = 0;
                        {
                            int64_t q = pv;
                            for (uint32_t rem = fl; rem; ) {
                                const int bit = __clz((int)rem);
                                rem &= ~(0x80000000u >> bit);
                                const int64_t fa = p + bit;
                                const uint64_t adv = sqzr_advance(sqzr_run(file, len, fa, q));
                                if (!sum) first_adv = adv;
                                sum += adv; q = fa;
                            }
                        }
                        uint64_t exB, totB;
                        block_scan(sum, OpAdd(), &exB, &totB, s_w);
                        const uint64_t cum0 = carry_sum + exB;
                        if (tid == 0) s_over = 0xFFFFFFFFu;
                        const bool any = __syncthreads_or(cnt != 0u && cum0 + first_adv - 1u < (uint64_t)n) != 0;
                        if (any && !mat) {                          // the first take of the band: the LIP becomes an array
                            for (uint32_t k = tid; k < n; k += kT) lip[k] = scan_entry(b, k);
                            mat = true;
                            __syncthreads();
                        }
                        {
                            int64_t q = pv;
                            uint64_t cum = cum0;
                            uint32_t rank = (uint32_t)(exA >> 32);
                            for (uint32_t rem = fl; rem; ) {
                                const int bit = __clz((int)rem);
                                rem &= ~(0x80000000u >> bit);
                                const int64_t fa = p + bit;
                                cum += sqzr_advance(sqzr_run(file, len, fa, q));
                                if (cum - 1u >= (uint64_t)n) { atomicMin(&s_over, (uint32_t)(fa - P) << 16 | rank); break; }
                                const uint32_t t = (uint32_t)(cum - 1u);
                                const uint32_t xy = lip[t];
                                lip[t] = kSqzrTaken;
                                lsp[lspn + nsp + rank] = xy;
                                int16_t* c = coef_at(coeffs, b, xy);
                                *c = (int16_t)(uint16_t)((uint32_t)(uint16_t)*c | mask | sqzr_sign(file, len, q));
                                ++rank; q = fa;
                            }
                        }
                        __syncthreads();
                        const uint32_t ov = s_over;
                        if (ov != 0xFFFFFFFFu) { nsp += ov & 0xFFFFu; pos = P + (int64_t)(ov >> 16) + 1; closed = true; break; }
                        nsp += (uint32_t)(totA >> 32);
                        carry_sum += totB;
                        if ((uint32_t)totA) carry_prev = P + (int64_t)(uint32_t)totA - 1;
                    }
                    if (!closed) pos = N;                           // the stream ended inside the pass: what was closed is applied, nothing is merged
                    go = pos < N;
                    if (go && nsp) {                                // the taken entries leave the LIP
                        uint32_t out = 0;
                        for (uint32_t base = 0; base < n; base += kT * kCompact) {
                            uint32_t e[kCompact], alive = 0;
                            #pragma unroll
                            for (int j = 0; j < kCompact; ++j) {
                                const uint32_t k = base + tid * kCompact + (uint32_t)j;
                                e[j] = k < n ? lip[k] : kSqzrTaken;
                                alive += e[j] != kSqzrTaken;
                            }
                            uint64_t ex, tot;
                            block_scan((uint64_t)alive, OpAdd(), &ex, &tot, s_w);
                            uint32_t w = out + (uint32_t)ex;
                            #pragma unroll
                            for (int j = 0; j < kCompact; ++j) if (e[j] != kSqzrTaken) lip[w++] = e[j];
                            out += (uint32_t)tot;
                        }
                    }
                }
                if (go) {                                           // the refinement pass :2039-2057
                    const uint64_t m = sqzr_refine_bits(lspn, pos, N);
                    const uint32_t rmask = 1u << (bp & 15);
                    const uint64_t groups = (m + 31u) / 32u;
                    for (uint64_t g = tid; g < groups; g += kT) {
                        uint32_t w = sqzr_bits32(file, len, pos + (int64_t)(32u * g));
                        const uint64_t valid = m - 32u * g;
                        if (valid < 32u) w &= ~(0xFFFFFFFFu >> valid);
                        while (w) {
                            const int bit = __clz((int)w);
                            w &= ~(0x80000000u >> bit);
                            int16_t* c = coef_at(coeffs, b, lsp[32u * g + (uint32_t)bit]);
                            *c = (int16_t)(uint16_t)((uint32_t)(uint16_t)*c | rmask);
                        }
                    }
                    pos += (int64_t)m;
                    go = m == (uint64_t)lspn && pos < N;
                }
                if (go) bp -= bp > 0;                               // a completed visit: the NSP is merged
                if (tid == 0) {
                    s_max[slot] = (int8_t)mx; s_bp[slot] = (int8_t)bp; s_mat[slot] = mat;
                    if (go) { s_lspn[slot] = lspn + nsp; s_lipn[slot] = n - nsp; }
                }
                __syncthreads();
                if (!go) { stop = true; break; }
                done = done && bp == 0;
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
    __syncthreads();
    // SQZ_decode_round_coefficients :2082-2103: the merged entries alone
    for (int slot = 0; slot < kSqzSlots; ++slot) {
        const uint32_t rm = sqzr_round_mask(s_max[slot], s_bp[slot]), cnt = s_lspn[slot];
        if (!rm || !cnt) continue;
        const RBand b = B[slot];
        const uint32_t* lsp = lsp_all + b.list_base;
        for (uint32_t k = tid; k < cnt; k += kT) {
            int16_t* c = coef_at(coeffs, b, lsp[k]);
            *c = (int16_t)(uint16_t)((uint32_t)(uint16_t)*c | rm);
        }
    }
}

thread_local float t_read_ms[2] = { -1.0f, -1.0f };

std::atomic<int>& reader_switch()
{
    static std::atomic<int> r{ [] { const char* e = getenv("GAMUT_HIP_SQZ_READER"); return e && !strcmp(e, "device") ? 1 : 0; }() };
    return r;
}
std::atomic<int64_t>& chunk_limit()
{
    static std::atomic<int64_t> c{ (int64_t)1 << 31 };
    return c;
}

struct Reader {
    DeviceScratch blob, lists;
    PinnedScratch pinned;
};

struct Job {
    const uint8_t* const* data; const size_t* len; const gamut_hip_sqz_info* info; const int* which;
    int16_t* coeffs; const int64_t* coeff_offset; hipStream_t stream; bool timing;
};

int read_chunk(Reader& R, SqzScanTables& T, const Job& J, size_t a, size_t b)
{
    const size_t n = b - a, nb = n * kSqzSlots;
    hipStream_t stream = J.stream;
    const TracePoint t_tab = trace_now();
    const size_t o_bands = 0, o_imgs = o_bands + up256(nb * sizeof(RBand)), o_files = o_imgs + up256(n * sizeof(RImg));
    size_t total = o_files;
    std::vector<size_t> foff(n);
    for (size_t k = 0; k < n; ++k) { foff[k] = total - o_files; total += up16(J.len[J.which[a + k]]); }
    uint8_t* d = (uint8_t*)R.blob.get(total, stream);
    uint8_t* h = R.pinned.get(total, stream);
    if (!d || !h) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_read: %zu bytes of tables and files could not be had", total);
    memset(h, 0, o_files);
    RBand* hb = (RBand*)(h + o_bands); RImg* hi = (RImg*)(h + o_imgs);
    uint64_t elems = 0;
    for (size_t k = 0; k < n; ++k) {
        const int i = J.which[a + k];
        const gamut_hip_sqz_info& I = J.info[i];
        gamut_hip_sqz_encode_desc D{};
        D.width = I.width; D.height = I.height; D.color_mode = I.color_mode; D.levels = I.levels; D.scan_order = I.scan_order; D.subsampling = I.subsampling;
        SqzBandGeom g[kSqzSlots];
        sqz_band_geometry(D, g);
        for (int s = 0; s < kSqzSlots; ++s) {
            RBand& B = hb[k * kSqzSlots + (size_t)s];
            B.round = g[s].round;
            if (!g[s].width) continue;
            B.n = g[s].width * g[s].height; B.bw = g[s].width; B.stride = g[s].stride;
            B.coeff_off = J.coeff_offset[i] + g[s].offset; B.list_base = elems;
            elems += ((uint64_t)B.n + 3u) & ~(uint64_t)3u;
            if (I.scan_order != 0 && !(B.table = T.table(I.scan_order, g[s].width, g[s].height))) return GAMUT_HIP_ERR_OUT_OF_MEMORY;
        }
        hi[k] = RImg{ (uint64_t)foff[k], (uint64_t)J.len[i], J.coeff_offset[i], (uint64_t)I.width * (uint64_t)I.height * (uint64_t)I.planes, (uint32_t)I.planes, (uint32_t)I.levels };
    }
    parallel_for((int)n, std::min(std::min(host_threads(), 16), (int)n), [&](int, int k) {
        const int i = J.which[a + (size_t)k];
        memcpy(h + o_files + foff[(size_t)k], J.data[i], J.len[i]);
    });
    uint32_t* lists = (uint32_t*)R.lists.get((size_t)(elems * 2u + 8u) * sizeof(uint32_t), stream);
    if (!lists) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_read: %llu bytes of list scratch could not be had", (unsigned long long)elems * 8u);
    StreamDrain drain;
    GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, total, hipMemcpyHostToDevice, stream));
    drain.arm(stream);
    if (J.timing) t_read_ms[1] += (float)ms_since(t_tab);
    float ms = 0;
    {
        KernelTimer<2> timer(J.timing);
        timer.mark(stream);
        hipLaunchKernelGGL(k_sqzr_zero, dim3(kZeroX, (unsigned)n), dim3(kZeroThreads), 0, stream, (const RImg*)(d + o_imgs), J.coeffs);
        hipLaunchKernelGGL(k_sqzr_walk, dim3((unsigned)n), dim3(kT), 0, stream, (const RBand*)(d + o_bands), (const RImg*)(d + o_imgs), (const uint8_t*)(d + o_files),
                           J.coeffs, lists, lists + elems);
        if (int rc = launch_status("sqz_read")) return rc;
        timer.mark(stream);
        const hipError_t e = drain.wait();
        if (e != hipSuccess) return set_error(GAMUT_HIP_ERR_HIP, "sqz_read: %s", hipGetErrorString(e));
        timer.finish(&ms);
    }
    if (J.timing) t_read_ms[0] = ms < 0 || t_read_ms[0] < 0 ? -1.0f : t_read_ms[0] + ms;
    return GAMUT_HIP_OK;
}

} // namespace

int sqz_reader() { return reader_switch().load(std::memory_order_relaxed); }

// For i in which[]: file (data[i], len[i]) has passed sqz_parse_header into info[i]; its coefficients go to DEVICE memory at
// coeffs + coeff_offset[i].  Returns when they are in place; anything but GAMUT_HIP_OK is a failure of the call, not of a file.
int sqz_read_files(const uint8_t* const* data, const size_t* len, const gamut_hip_sqz_info* info, const std::vector<int>& which,
                   int16_t* coeffs, const int64_t* coeff_offset, hipStream_t stream)
{
    static const bool timing = env_flag("GAMUT_HIP_SQZ_TIMING");
    static thread_local PerDevice<Reader> reader_pd;
    if (which.empty()) return GAMUT_HIP_OK;
    Reader& R = reader_pd.cur();
    SqzScanTables& T = sqz_scan_tables();
    if (T.table_bytes > kSqzTableCap) T.drop_tables();
    if (timing) t_read_ms[0] = t_read_ms[1] = 0.0f;
    const uint64_t limit = (uint64_t)chunk_limit().load(std::memory_order_relaxed);
    const Job J{ data, len, info, which.data(), coeffs, coeff_offset, stream, timing };
    for (size_t a = 0; a < which.size(); ) {
        size_t b = a; uint64_t elems = 0;
        while (b < which.size() && b - a < kChunkFiles) {
            const gamut_hip_sqz_info& I = info[which[b]];
            const uint64_t e = (uint64_t)I.width * (uint64_t)I.height * (uint64_t)I.planes;
            if (b > a && elems + e > limit) break;
            elems += e; ++b;
        }
        if (int rc = read_chunk(R, T, J, a, b)) return rc;
        a = b;
    }
    return GAMUT_HIP_OK;
}

} // namespace gamut

using namespace gamut;

extern "C" {

int gamut_hip_sqz_read_batch_device(const uint8_t* const* data, const size_t* len, int count, int16_t* coeffs, const int64_t* coeff_offset,
                                    gamut_hip_sqz_info* info, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!data || !len || !coeffs || !coeff_offset)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_read_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        std::vector<gamut_hip_sqz_info> hd((size_t)count);
        std::vector<int> which;
        SqzRefusals bad; bad.status = status_host;
        for (int i = 0; i < count; ++i) {
            if (status_host) status_host[i] = GAMUT_HIP_OK;
            int rc = sqz_parse_header(data[i], len[i], &hd[(size_t)i]);
            if (info) info[i] = hd[(size_t)i];
            if (rc == GAMUT_HIP_OK && coeff_offset[i] < 0) rc = set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: negative coeff_offset");
            if (rc != GAMUT_HIP_OK) { bad.refuse(i, rc); continue; }
            which.push_back(i);
        }
        if (int rc = sqz_read_files(data, len, hd.data(), which, coeffs, coeff_offset, pick_stream(stream))) return rc;
        return bad.verdict();
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_read_batch_device: out of host memory");
    }
}

int gamut_hip_sqz_set_reader(int which)
{
    if (which != 0 && which != 1) return reader_switch().load(std::memory_order_relaxed);
    return reader_switch().exchange(which, std::memory_order_relaxed);
}

int gamut_hip_sqz_read_window(void) { return kWindow; }

int64_t gamut_hip_sqz_set_read_chunk(int64_t coefficients)
{
    if (coefficients < 1) return chunk_limit().load(std::memory_order_relaxed);
    return chunk_limit().exchange(coefficients, std::memory_order_relaxed);
}

float gamut_hip_sqz_last_read_stage_ms(int stage) { return stage >= 0 && stage < 2 ? t_read_ms[stage] : -1.0f; }

} // extern "C"
