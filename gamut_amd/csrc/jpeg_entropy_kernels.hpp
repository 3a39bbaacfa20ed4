// jpeg_entropy_kernels.hpp -- the device structs and the kernels of the baseline entropy decode (k_jpeg_entropy, k_jpeg_entropy_sync,
// k_jpeg_unstuff).  Included by jpeg_host.hip inside its namespace, behind jpeg_parse.hpp; jpeg_batch.hpp launches what is here.
// =====================================================================================================================
// Entropy decode ON THE GPU: baseline scans only.
//
// Huffman decoding is serial inside a stream, but a batch holds many independent streams: every image, and inside an
// image every restart interval (process_restart :2335-2402 resets the DC predictors and byte-aligns the stream), can be
// decoded by its own lane.  The host only walks the markers (tables, geometry) and locates the RSTn boundaries; the
// compressed bytes go to the device as they are (230 kB instead of 6.3 MB of coefficients per 1080p image over PCIe) and
// k_jpeg_entropy writes the same dense de-quantised coefficient form decode_next_row (:2405-2525) produces, straight
// into HBM, ready for k_jpeg_h2v2 / k_jpeg_generic.  Same arithmetic as decode_baseline() above, which is its oracle.
#ifndef JPEG_HUFF_SUB_ENTRIES      // (tools/variant.sh knob; the standard tables need 144 / 150 entries)
#define JPEG_HUFF_SUB_ENTRIES 312      // sizeof(DevHuff) = 2048: a table's address is a shift of its number
#endif
struct DevHuff {                       // one Huffman table (shared by every image that uses the same table)
    uint16_t fast[512];                // 9-bit lookahead -> (length << 8) | symbol, 0 = longer code
    int32_t  maxcode[18];
    int32_t  delta[17];
    uint8_t  vals[256];
    uint8_t  pad[4];
    // codes of more than 9 bits, second level: fast[p] of a 9-bit prefix p that only longer codes begin with = 0x8000 | x << 12 | offset: the next
    // x bits (x = the longest such code's length - 9, 1 .. 7) index sub[offset ..] -> (length << 8) | symbol, 0 = no such code.  A table whose
    // second levels do not fit in sub[] keeps fast[p] = 0 for the prefixes that did not (and the canonical search over maxcode[] finds the code,
    // as it did for every long code before round 4: up to eight dependent LDS reads, and with 64 lanes per wave SOME lane has a long code in most steps).
    uint16_t sub[JPEG_HUFF_SUB_ENTRIES];
};
constexpr uint32_t kHuffLong = 0x8000u;
static_assert(JPEG_HUFF_SUB_ENTRIES != 312 || sizeof(DevHuff) == 2048, "DevHuff: a power of two");
inline void to_dev_huff_build(const HuffTable& h, DevHuff& d);
inline void to_dev_huff(const HuffTable& h, DevHuff& d)      // (the same few tables file after file: the last ones a thread converted are kept, as in the DHT walk)
{
    struct Made { bool used = false; uint8_t bits[17]; uint8_t vals[256]; DevHuff d; };
    constexpr int kKept = 32;
    static thread_local std::unique_ptr<Made[]> cache; static thread_local unsigned victim = 0;
    if (!cache) cache.reset(new Made[kKept]);
    for (int k = 0; k < kKept; ++k) if (cache[k].used && !memcmp(cache[k].bits, h.bits, sizeof(h.bits)) && !memcmp(cache[k].vals, h.vals, sizeof(h.vals))) { d = cache[k].d; return; }
    to_dev_huff_build(h, d);
    Made& m = cache[victim++ % kKept];
    memcpy(m.bits, h.bits, sizeof(m.bits)); memcpy(m.vals, h.vals, sizeof(m.vals)); m.d = d; m.used = true;
}
inline void to_dev_huff_build(const HuffTable& h, DevHuff& d)
{
    memset(&d, 0, sizeof(d));
    for (int w = 0; w < 512; ++w) { const uint16_t e = h.fast[w << 1]; d.fast[w] = (e >> 8) <= 9 ? e : 0; }   // 10-bit table -> 9-bit
    memcpy(d.maxcode, h.maxcode, sizeof(d.maxcode)); memcpy(d.delta, h.delta, sizeof(d.delta)); memcpy(d.vals, h.vals, sizeof(d.vals));
    // second level: the longest code under every 9-bit prefix, then the codes themselves (canonical order: bits[] / vals[])
    uint8_t longest[512] = { 0 };
    int code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < h.bits[len]; ++i, ++code) if (len > 9) { uint8_t& m = longest[(code >> (len - 9)) & 511]; if (len > m) m = (uint8_t)len; }
        code <<= 1;
    }
    int used = 0;
    uint16_t off[512];
    for (int p = 0; p < 512; ++p) {
        off[p] = 0xFFFF;
        if (!longest[p] || d.fast[p]) continue;                  // (a prefix shorter codes cover cannot begin a longer one: the table is a prefix code)
        const int n = 1 << (longest[p] - 9);
        if (used + n > (int)(sizeof(d.sub) / sizeof(d.sub[0]))) continue;
        off[p] = (uint16_t)used; used += n;
        d.fast[p] = (uint16_t)(kHuffLong | (uint32_t)(longest[p] - 9) << 12 | off[p]);
    }
    code = 0; k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < h.bits[len]; ++i, ++code, ++k) {
            if (len <= 9) continue;
            const int p = (code >> (len - 9)) & 511;
            if (off[p] == 0xFFFF) continue;
            const int x = longest[p] - 9, have = len - 9;         // the code's bits behind the prefix, left-aligned in the x index bits
            const int first = (code & ((1 << have) - 1)) << (x - have), n = 1 << (x - have);
            for (int j = 0; j < n; ++j) d.sub[off[p] + first + j] = (uint16_t)((len << 8) | h.vals[k]);
        }
        code <<= 1;
    }
}
struct DevImage {
    int64_t coeff_off, zag_off;        // int16 elements / bytes from the start of the caller's buffers
    int32_t nb, org;                   // blocks per MCU; component of block b = (org >> 2 * b) & 3: the order the SOS lists them in (scan_block_order)
    int32_t quant[3], dc[3], ac[3];    // table indices per component
    int32_t tok;                       // 1: the coefficients leave as a token stream (compact hand-off, below) instead of dense 128-byte blocks
    int64_t tok_off, strip_off;        // the image's tokens / strip table: elements from the start of the token buffer / the strip-start buffer
    int32_t sb, row_blocks;            // blocks per strip of the reconstruction kernel (k_jpeg_h2v2: 8 MCUs = 48), blocks per MCU row
    int32_t n_strips, tok_cap;         // strips of the image (its table has n_strips + 1 entries), tokens its slot holds
};
constexpr uint32_t kStatusBadRestart = 8u;
struct DevItem { int32_t image, first_mcu, n_mcus, pad; uint64_t begin, end; int32_t tail, pad2; };    // one restart interval (or whole scan)
// tail: -1 = nothing follows the segment but the end of the scan; >= 0 = an RSTn marker follows it, behind `tail` 0xFF fill bytes (restart_leftover_bad)

// process_restart (jpegload.d:2335-2402) does not look for the marker where the interval's data ENDS but from where the decoder's input
// stands: the bit reader holds 16 .. 32 bits, fetched two octets at a time (four at a (re)start) and never past a marker, so after
// `used_bits` bits of an interval the input is 4 + 2 * (used_bits / 16) octets behind the interval's start.  From there at most 1536 raw
// bytes are read up to a 0xFF, then its fill bytes, and what follows has to be the expected RSTn.  For an intact file that position IS the
// marker (an encoder pads the last byte and nothing more).  A damaged one may leave whole octets between the two: they are skipped if none
// of them is 0xFF (a stuffed FF 00 is "FF, then not RSTn": JPGD_BAD_RESTART_MARKER) and if they, the marker's 0xFF and its fill bytes are
// within the 1536 reads.  seg = the UNSTUFFED interval (every 0xFF in it was FF 00), seg_bytes its length, fill = 0xFF bytes between the
// marker's first 0xFF and its code.  (The markers themselves -- the wrong RSTn, a missing one -- are checked where the scan is unstuffed.)
__device__ inline bool restart_leftover_bad(const uint8_t* seg, uint32_t seg_bytes, uint32_t used_bits, int fill)
{
    const uint64_t oct = 4 + 2 * (uint64_t)(used_bits / 16);
    const uint32_t left = oct < seg_bytes ? seg_bytes - (uint32_t)oct : 0u;
    if (left + (uint32_t)fill > 1535u) return true;
    for (uint32_t i = 0; i < left; ++i) if (seg[oct + i] == 0xFF) return true;
    return false;
}

__constant__ uint8_t kZagDev[64] = { 0,1,8,16,9,2,3,10,17,24,32,25,18,11,4,5,12,19,26,33,40,48,41,34,27,20,13,6,7,14,21,28,35,42,49,56,57,50,43,36,29,22,15,23,30,37,44,51,58,59,52,45,38,31,39,46,53,60,61,54,47,55,62,63 };

// MSB-first reader over an UNSTUFFED segment (the host drops the 0x00 after every 0xFF while it copies the scan, and
// appends 64 bytes of 0xFF after each segment: reading past the end yields 1-bits, as get_octet :683-696 does, and an
// all-ones window is no valid Huffman code, so a runaway decode of corrupt data stops within two bytes of the padding).
struct DevBits {
    const uint8_t* next;               // next four bytes to fetch
    uint64_t acc; int nbits; uint32_t pos;     // pos = bit index (from the segment start) of the next unread bit
    uint32_t pre;                      // bytes at `next`, requested one refill ahead: a lane is a serial chain of dependent
                                       // operations, so the global-memory latency has to overlap the symbols in between
    __device__ __forceinline__ void open(const uint8_t* seg, uint32_t bit)
    {
        next = seg + (bit >> 3); acc = 0; nbits = 0; pos = bit;
        __builtin_memcpy(&pre, next, 4);
        refill();
        nbits -= (int)(bit & 7);                              // drop the bits before `bit` in its byte
    }
    __device__ __forceinline__ void refill()
    {
        if (nbits > 32) return;
        acc = (acc << 32) | __builtin_bswap32(pre); nbits += 32; next += 4;
        __builtin_memcpy(&pre, next, 4);
    }
    __device__ __forceinline__ uint32_t peek(int n) const { return (uint32_t)(acc >> (nbits - n)) & ((1u << n) - 1); }
    __device__ __forceinline__ void drop(int n) { nbits -= n; pos += (uint32_t)n; }
    __device__ __forceinline__ int decode(const DevHuff* h)
    {
        refill();
        const uint32_t e = h->fast[peek(9)];
        if (e && e < kHuffLong) { drop((int)(e >> 8)); return (int)(e & 0xFF); }
        if (e) {                                                // a longer code: the second level (DevHuff.sub)
            const int xb = (int)(e >> 12) & 7;
            const uint32_t e2 = h->sub[(e & 0xFFFu) + (peek(9 + xb) & ((1u << xb) - 1u))];
            if (e2) { drop((int)(e2 >> 8)); return (int)(e2 & 0xFF); }
        }
        int32_t code = (int32_t)peek(9); int len = 9;
        while (code > h->maxcode[len]) { if (++len > 16) return -1; code = (int32_t)peek(len); }
        drop(len);
        return h->vals[(code + h->delta[len]) & 0xFF];
    }
    __device__ __forceinline__ int receive_extend(int s)       // JPGD_HUFF_EXTEND :816-822
    {
        if (!s) return 0;
        refill();
        const int v = (int)peek(s); drop(s);
        return v < (1 << (s - 1)) ? v + (int)(0xFFFFFFFFu << s) + 1 : v;
    }
};

constexpr size_t kBlobSlack = 1024;                          // bytes a lane may read past the last segment: one block + look-ahead in k_jpeg_entropy; in k_prog_scan the 64-byte limit check + a block's worth of a corrupt AC scan (244 bytes) + the 256-byte window
#ifndef JPEG_HUFF_SUB              // A/B knob (tools/variant.sh jpeg_host:nosub:-DJPEG_HUFF_SUB=0): 0 = no second-level Huffman look-up in sub_decode
#define JPEG_HUFF_SUB 1
#endif
// Lanes per long segment.  A group of 256 files is 256 workgroups -- one per compute unit: with 256 lanes that is ONE wave per SIMD, a chain of
// dependent instructions at 8 clocks each (tools/microbench/chain_latency.hip) over 880 bytes per lane and pass.  512 lanes: half the bytes per
// lane, two waves per SIMD to alternate between; the passes to the fixed point grow by less.  Round 4, one box, rocprofv3: the compact kernel
// 3.49 -> 2.80 ms per group of 256 files (1024 lanes: 2.99), files -> pixels 256 files 5.9-6.7 -> 5.0-5.1 ms; 1024 files (inside the run-to-run
// spread), 4096 files and the mixed call unchanged (there the GPU is full either way) -- profiles/r04_jpeg_sync_lanes.txt.
#ifndef JPEG_SYNC_THREADS          // tuning knob (tools/variant.sh)
#define JPEG_SYNC_THREADS 512
#endif
constexpr int kEntropyThreads = 64;                          // one wave per workgroup: lanes spread over CUs, each with its own L1
constexpr int kLdsHuff = JPEG_SYNC_THREADS >= 1024 ? 4 : 8, kLdsQuant = kLdsHuff;                     // tables a workgroup keeps in LDS (15 KB + 1 KB: two encoders' sets; more distinct tables in a batch are read from global memory)
constexpr int kSyncThreads = JPEG_SYNC_THREADS;                // lanes cooperating on one large segment
constexpr uint32_t kSyncMinBytes = 4096;                       // shorter segments take one lane each

// Tables into LDS (IN_LDS: the batch uses few distinct tables -- the usual case: encoders write the Annex K tables or one
// optimised set per quality -- so a symbol costs LDS latencies instead of L2 ones; the look-up sits on the lane's
// critical path twice per symbol).
template <bool IN_LDS, int NT>
__device__ __forceinline__ void load_tables(DevHuff* sh_huff, int16_t* sh_quant, uint8_t* sh_zag, const DevHuff* huff_g, int n_huff,
                                            const int16_t* quant_g, int n_quant)
{
    if (threadIdx.x < 64) sh_zag[threadIdx.x] = kZagDev[threadIdx.x];
    if constexpr (IN_LDS) {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(huff_g); uint32_t* dst = reinterpret_cast<uint32_t*>(sh_huff);
        for (int k = threadIdx.x; k < n_huff * (int)(sizeof(DevHuff) / 4); k += NT) dst[k] = src[k];
        for (int k = threadIdx.x; k < n_quant * 64; k += NT) sh_quant[k] = quant_g[k];
    }
}

// ---- one lane per (short) segment -------------------------------------------------------------------------------
template <bool IN_LDS>
__global__ __launch_bounds__(kEntropyThreads) void k_jpeg_entropy(const DevItem* items, int n_items, const DevImage* images,
                                                                  const DevHuff* huff_g, int n_huff, const int16_t* quant_g /* [t][64], zig-zag order */,
                                                                  int n_quant, const uint8_t* blob, int16_t* coeffs, uint8_t* max_zag, uint32_t* status)
{
    __shared__ DevHuff sh_huff[IN_LDS ? kLdsHuff : 1];
    __shared__ int16_t sh_quant[IN_LDS ? kLdsQuant * 64 : 1];
    __shared__ uint8_t sh_zag[64];
    // The block being decoded lives in LDS (one 128-byte row per lane, 144-byte pitch): the sparse coefficient writes are
    // LDS writes, and a finished block leaves as eight 16-byte stores -- a whole line, zeros included, so the destination
    // needs no clearing and the lane's bit-stream loads never queue behind a trail of 2-byte global stores.
    __shared__ __attribute__((aligned(16))) uint8_t sh_blk[kEntropyThreads * 144];
    load_tables<IN_LDS, kEntropyThreads>(sh_huff, sh_quant, sh_zag, huff_g, n_huff, quant_g, n_quant);
    {
        uint4* z = reinterpret_cast<uint4*>(sh_blk + threadIdx.x * 144);
        #pragma unroll
        for (int k = 0; k < 8; ++k) z[k] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    const DevHuff* huff = IN_LDS ? sh_huff : huff_g;
    const int16_t* quant = IN_LDS ? sh_quant : quant_g;

    const int i = blockIdx.x * kEntropyThreads + threadIdx.x;
    if (i >= n_items) return;
    const DevItem it = items[i];
    const DevImage im = images[it.image];
    DevBits br; br.open(blob + it.begin, 0);
    // A lane may run past its segment only by the 64 bytes of 0xFF padding: with the standard (incomplete) tables an
    // all-ones window is no code and the decode stops by itself, but a DHT may define a COMPLETE code (all-ones included),
    // and a truncated scan under a large SOF would then keep "decoding" padding, the next segments and whatever follows the
    // blob.  Checked once per block: a block consumes < 256 bytes, and the blob is allocated with that much slack.
    const uint32_t limit_bit = (uint32_t)(it.end - it.begin) * 8u + 64u * 8u;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    int16_t* out = coeffs + im.coeff_off + (int64_t)it.first_mcu * im.nb * 64;
    uint8_t* mz = max_zag + im.zag_off + (int64_t)it.first_mcu * im.nb;
    int16_t* blk = reinterpret_cast<int16_t*>(sh_blk + threadIdx.x * 144);
    // damaged data: flag the image and clear the blocks of the segment that were not reached (the caller's buffer is not cleared beforehand)
    int16_t* const seg_end = out + (int64_t)it.n_mcus * im.nb * 64;
    auto bail = [&](uint32_t flag) {
        atomicOr(status + it.image, flag);
        for (int16_t* p = out; p < seg_end; p += 64) {
            uint4* dst = reinterpret_cast<uint4*>(p);
            #pragma unroll
            for (int k = 0; k < 8; ++k) dst[k] = make_uint4(0, 0, 0, 0);
        }
    };
    for (int mcu = 0; mcu < it.n_mcus; ++mcu) {
        for (int b = 0; b < im.nb; ++b, out += 64, ++mz) {
            const int c = (int)((uint32_t)im.org >> (2 * b)) & 3;
            const int16_t* q = quant + (c == 0 ? im.quant[0] : c == 1 ? im.quant[1] : im.quant[2]) * 64;
            const DevHuff* dc = huff + (c == 0 ? im.dc[0] : c == 1 ? im.dc[1] : im.dc[2]);
            const DevHuff* ac = huff + (c == 0 ? im.ac[0] : c == 1 ? im.ac[1] : im.ac[2]);
            const int s = br.decode(dc);
            if (s < 0) { bail(1u); return; }
            const int pred = c == 0 ? pred0 : c == 1 ? pred1 : pred2;
            const int v = br.receive_extend(s & 15) + pred;
            if (c == 0) pred0 = v; else if (c == 1) pred1 = v; else pred2 = v;
            blk[0] = (int16_t)((uint32_t)v * (uint32_t)(int32_t)q[0]);
            int kk = 1;
            for (; kk < 64; ++kk) {
                const int rs = br.decode(ac);
                if (rs < 0) { bail(1u); return; }
                const int run = rs >> 4, size = rs & 15;
                if (size) {
                    if (run) { if (kk + run > 63) { bail(2u); return; } kk += run; }
                    const int e = br.receive_extend(size);
                    blk[sh_zag[kk]] = (int16_t)((uint32_t)e * (uint32_t)(int32_t)q[kk]);
                } else if (run == 15) {
                    if (kk + 16 > 64) { bail(2u); return; }
                    kk += 15;
                } else break;
            }
            if (br.pos > limit_bit) { bail(4u); return; }                               // ran off the end of the segment
            *mz = (uint8_t)kk;                                   // m_mcu_block_max_zag :2512
            uint4* src = reinterpret_cast<uint4*>(blk);
            uint4* dst = reinterpret_cast<uint4*>(out);          // 128-byte blocks at 128-byte-aligned offsets (checked by the host)
            #pragma unroll
            for (int k = 0; k < 8; ++k) { dst[k] = src[k]; src[k] = make_uint4(0, 0, 0, 0); }
        }
    }
    if (it.tail >= 0 && restart_leftover_bad(blob + it.begin, (uint32_t)(it.end - it.begin), br.pos, it.tail)) atomicOr(status + it.image, kStatusBadRestart);
}

// ---- many lanes per (long) segment: self-synchronising decode --------------------------------------------------------
// A Huffman stream can only be entered at a codeword boundary in a known state -- here (bit position, block of the MCU,
// zig-zag index) -- which only a decoder that came from the start knows.  But decoders started at the WRONG place fall
// into step with the right one after a few symbols (Huffman codes self-synchronise; cf. Weissenberger & Schmidt's
// parallel JPEG decoding).  A workgroup cuts its segment into one sub-sequence per lane; lane t decodes from the state
// lane t-1 LEFT its sub-sequence with and records the state it leaves its own with; this is repeated until no recorded
// exit state changes.  Lane 0 starts from the true state, so the fixed point is the true decode (induction over t).  Lanes
// whose entry state did not change keep their result, so after the first two sweeps only the few unsettled ones work.
// Then block counts and DC differences are prefix-summed across lanes and one last sweep writes the coefficients.
struct SubState { uint32_t pos; uint16_t c, z; };
__device__ __forceinline__ bool same(const SubState& a, const SubState& b) { return a.pos == b.pos && a.c == b.c && a.z == b.z; }

struct SubCtx {
    const DevHuff* huff; const int16_t* quant; const uint8_t* zag;
    const uint8_t* seg; uint32_t end_bit;
    const int* par;                     // LDS: [component] -> quant table, DC table, AC table (3 x 3 ints), the segment's image
    uint32_t org; int nb;              // org: DevImage.org
};

// Decode from state `s` while the position is inside this lane's sub-sequence.  WRITE: coefficients / max_zag go out,
// starting in block `b` with DC predictors pred[]; otherwise only the exit state, the number of blocks finished and the
// sums of the DC differences are produced.  Returns false on a stream error (only meaningful on the true path).
// The 64 lanes of a wave are at 64 different places of the token grammar (DC or AC symbol, short or long code, coefficient / ZRL /
// EOB, end of a block or not), so every branch of a symbol step is taken by SOME lane and a branchy step costs the sum of its
// paths (430 instructions as first written, half of them exec-mask bookkeeping).  The step is therefore straight-line: one refill
// (33 bits cover the longest code plus the longest value), the table picked by index, every outcome a predicate, the new state a
// handful of selects; only the rare long code (> 9 bits) and the stores are under a mask.
// MODE 0: only the exit state, the blocks finished and the DC sums.  MODE 1 (the write sweep): a block this lane STARTS is
// assembled in the lane's 128 bytes of LDS (`blk`, zero on entry) and leaves as one whole line when it ends -- or, unfinished, when
// the sub-sequence ends (its remaining coefficients belong to the lanes after this one); a block the lane finds half-decoded at its
// entry (z > 0) is only counted here.  MODE 2 (after a barrier): exactly that first, inherited block again, its coefficients stored
// one by one on top of the line its starter wrote.  Scattered 2-byte stores for everything (the first version, into a buffer
// cleared beforehand) cost 13 GB of HBM traffic per 512 images for 3 GB of coefficients: every store a read-modify-write of a line.
enum { SUB_COUNT = 0, SUB_WRITE = 1, SUB_FIRST = 2, SUB_TOKENS = 3 };
// SUB_TOKENS (round 4, the compact hand-off): the write sweep emits one 4-byte TOKEN per coefficient instead of assembling 128-byte
// blocks -- [31:26] block of the reconstruction kernel's strip, [25:20] natural position, [15:0] the de-quantised value -- every DC and
// every non-zero AC coefficient, in stream order, so the tokens of consecutive lanes are consecutive (a lane's first token index comes
// from a fifth prefix sum) and a block split between lanes needs no second pass.  The strips of the reconstruction kernel are runs of
// consecutive blocks of the stream: the lane that starts a strip's first block records where the strip's tokens begin, and the kernel
// (k_jpeg_h2v2<.., TOK>) scatters the tokens of its strip into the LDS tile it used to load from memory.  A lane collects its tokens
// in 64 bytes of LDS and ships them every 16 steps, all lanes at once (four 16-byte stores at most): shipping whole 128-byte lines the
// moment a block ended was 1.6 M of the write sweep's 4.5 M cycles per file, and a q 90 block is ~12 tokens = 48 bytes.
struct TokCtx {
    uint32_t* out;                      // this lane's region of the image's token stream
    uint32_t* lds;                      // 16 dwords of staging
    uint32_t* strip_start;              // the image's strip table
    uint32_t base, total;               // index of the lane's first token in the image's stream; tokens the lane emits (from the counting pass)
    uint32_t emitted, nl;               // shipped so far; waiting in LDS
    int sb, SB, left_in_row, row_blocks;    // block of the current strip, blocks per strip, blocks left in the MCU row
    uint32_t strip, n_strips;
    __device__ __forceinline__ void flush()
    {
        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
        struct __attribute__((packed, aligned(4))) V4 { u32x4 v; };
        #pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (nl > (uint32_t)(4 * p)) {
                const u32x4 v = *reinterpret_cast<const u32x4*>(lds + 4 * p);
                uint32_t* dst = out + emitted + 4 * p;
                if (emitted + 4 * p + 4 <= total) reinterpret_cast<V4*>(dst)->v = v;        // (the tail past nl is this lane's own: the next flush rewrites it)
                else { for (uint32_t k = 0; k < 4 && emitted + 4 * p + k < total && 4 * p + k < nl; ++k) dst[k] = v[k]; }   // the lane's last dwords: exactly
            }
        }
        emitted += nl; nl = 0;
    }
};
// Checkpoints of a counting pass: the decoder's state and running totals the first time it stands at or behind byte j * ck_step of
// its sub-sequence.  A lane that decodes its sub-sequence AGAIN (its entry state changed) falls into step with its previous pass
// after a few symbols, like every Huffman decoder; from the first checkpoint where both passes stand in the same state the rest
// is the previous pass word for word -- the lane stops there and keeps the old exit state and the old totals behind the
// checkpoint.  Without this every re-decode ran its whole sub-sequence again (3.2 full counting passes per file on average; now
// one and a fraction).  kSubCk checkpoints per lane live in the write sweep's block staging area (not in use before that sweep).
// 16 bytes each: the DC sums modulo 2^16 as well -- only differences between two passes are used, and only the low 16 bits of a DC value reach its
// coefficient (an int16 product).  A lane's checkpoints share its piece of the staging area with the write sweep's block (dense hand-off: 144
// bytes, 9 checkpoints) or token buffer (compact hand-off: 64 bytes; the area is 80 bytes then, 5 checkpoints -- 29 KB of LDS per workgroup
// instead of 45, five workgroups per compute unit instead of three: the kernel is chains of dependent operations, what it lacks is waves).
constexpr int kSubCkMax = 9;
struct SubCk { uint32_t pos; uint16_t cz, nblk, ntok; int16_t dcs[3]; };         // cz = c | z << 4; nblk / ntok modulo 2^16 (only differences are used)
static_assert(sizeof(SubCk) == 16, "checkpoint size");
struct SubTrace {
    SubCk* ck;                      // this lane's checkpoints (LDS), or nullptr
    int n_ck;                       // how many
    uint32_t first_bit, step_bits;  // checkpoint j stands at bit first_bit + j * step_bits, j = 1 .. kSubCk
    bool compare;                   // a pass after the first: stop at a checkpoint that matches
    int old_nblk, old_dcs[3];       // the previous pass's totals
    int old_ntok, ntok;             // tokens (every DC, every non-zero AC coefficient): the previous pass's total; this pass's (out)
    bool stopped;                   // out: the pass ended at a matching checkpoint (exit state = the previous one)
    int stop_ck;                    // out: which one (measurement builds)
};
template <int MODE>
__device__ __forceinline__ bool sub_decode(const SubCtx& x, SubState& s, int& nblk, int (&dcs)[3], int64_t b, int64_t b_end,
                                           int16_t* out, uint8_t* mz, int16_t* blk = nullptr, SubTrace* tr = nullptr, TokCtx* tk = nullptr)
{
    constexpr bool WRITE = MODE != SUB_COUNT;
    DevBits br; br.open(x.seg, s.pos);
    int c = s.c, z = s.z;
    nblk = 0;
    bool ok = true;
    bool inherited = z > 0;                                                      // the block under way was started by another lane
    const int q0 = x.par[0], q1 = x.par[1], q2 = x.par[2];
    // (the table is picked by NUMBER and addressed by a shift: sizeof(DevHuff) is 2048.  Picking among six addresses kept apart by an empty asm
    //  cost the loads their address space -- flat loads with 64-bit addresses instead of ds_read -- and a multiply by 1936 is a quarter-rate instruction.)
    const int d0 = x.par[3], d1 = x.par[4], d2 = x.par[5], a0 = x.par[6], a1 = x.par[7], a2 = x.par[8];
    int dc0 = dcs[0], dc1 = dcs[1], dc2 = dcs[2];
    int ntok = 0;
    int ck_j = 0;                                                                // checkpoints passed
    uint32_t ck_next = 0xFFFFFFFFu;
    uint32_t steps = 0;
    if (MODE == SUB_COUNT && tr) { ck_next = tr->first_bit + tr->step_bits; tr->stopped = false; }
    while (br.pos < x.end_bit && (!WRITE || b < b_end)) {
        br.refill();                                                             // >= 33 bits: a code (<= 16) and its value (<= 15)
        const int comp = (int)(x.org >> (2 * c)) & 3;
        const bool is_dc = z == 0;
        const DevHuff* h = x.huff + (is_dc ? (comp == 0 ? d0 : comp == 1 ? d1 : d2) : (comp == 0 ? a0 : comp == 1 ? a1 : a2));
        const uint32_t top16 = br.peek(16);
        uint32_t e = h->fast[top16 >> 7];
#if !JPEG_HUFF_SUB
        if (e >= kHuffLong) e = 0;                                               // (A/B: the canonical search for every long code, as before round 4)
#endif
        if (e >= kHuffLong) {                                                    // a code of more than 9 bits: the second level
            const uint32_t xb = (e >> 12) & 7u;
            e = h->sub[(e & 0xFFFu) + ((top16 >> (7u - xb)) & ((1u << xb) - 1u))];
        }
        int len = (int)(e >> 8), sym = (int)(e & 0xFFu);
        bool bad = false;
        if (!e) {                                                                // no second level for this prefix, or no such code: the canonical search
            int32_t code = (int32_t)(top16 >> 7); len = 9;
            while (code > h->maxcode[len]) { if (++len > 16) break; code = (int32_t)(top16 >> (16 - len)); }
            bad = len > 16;                                                      // no such code: the block ends here, 16 bits are skipped
            sym = bad ? 0 : (int)h->vals[(code + h->delta[len > 16 ? 16 : len]) & 0xFF];
            len = bad ? 16 : len;
        }
        const int size = sym & 15, run = sym >> 4;
        const bool ac = !is_dc && !bad;
        const bool err_run = ac && size != 0 && run != 0 && z + run > 63;       // a coefficient beyond the block
        const bool zrl = ac && size == 0 && run == 15;
        const bool err_zrl = zrl && z + 16 > 64;
        const bool eob = ac && size == 0 && run != 15;
        const bool take = !bad && (is_dc || (size != 0 && !err_run));           // a coefficient (or DC difference) follows the code
        const int used = len + (take ? size : 0);
        const uint32_t raw = (uint32_t)(br.acc >> (br.nbits - used)) & ((1u << size) - 1u);
        const int ext = take && size ? ((int)raw < (1 << (size - 1)) ? (int)raw + (int)(0xFFFFFFFFu << size) + 1 : (int)raw) : 0;   // JPGD_HUFF_EXTEND :816-822
        br.drop(used);
        const int k = is_dc ? 0 : z + run;                                       // zig-zag position of that coefficient
        const int dcv = (comp == 0 ? dc0 : comp == 1 ? dc1 : dc2) + ext;
        const bool tdc = take && is_dc;
        dc0 = tdc && comp == 0 ? dcv : dc0; dc1 = tdc && comp == 1 ? dcv : dc1; dc2 = tdc && comp == 2 ? dcv : dc2;
        ntok += take ? 1 : 0;
        if (MODE == SUB_TOKENS) {
            if (is_dc && tk->sb == 0) tk->strip_start[tk->strip] = tk->base + tk->emitted + tk->nl;       // this block opens a strip: its tokens begin here
            if (take) {
                const int16_t qf = x.quant[(comp == 0 ? q0 : comp == 1 ? q1 : q2) * 64 + k];
                const uint32_t cv = (uint32_t)(uint16_t)(int16_t)((uint32_t)(is_dc ? dcv : ext) * (uint32_t)(int32_t)qf);
                tk->lds[tk->nl] = (uint32_t)tk->sb << 26 | (uint32_t)x.zag[k] << 20 | cv;
                ++tk->nl;
            }
        } else
        if (WRITE && take && (MODE == SUB_FIRST || !inherited)) {
            const int16_t qf = x.quant[(comp == 0 ? q0 : comp == 1 ? q1 : q2) * 64 + k];
            const int16_t cv = (int16_t)((uint32_t)(is_dc ? dcv : ext) * (uint32_t)(int32_t)qf);
            if (MODE == SUB_FIRST) out[b * 64 + x.zag[k]] = cv; else blk[x.zag[k]] = cv;
        }
        const int znew = take ? k + 1 : (zrl && !err_zrl) ? z + 16 : z;
        const bool full = !is_dc && znew == 64;
        const bool done = bad || err_run || err_zrl || eob || full;
        ok = ok && !(bad || err_run || err_zrl);
        if (MODE == SUB_TOKENS && done) {
            mz[b] = (uint8_t)(full ? 64 : z);                                    // m_mcu_block_max_zag :2512 (EOB: the position it was read at)
            ++tk->sb; --tk->left_in_row;
            if (tk->sb == tk->SB || tk->left_in_row == 0) { tk->sb = 0; ++tk->strip; }
            if (tk->left_in_row == 0) tk->left_in_row = tk->row_blocks;
            if (b + 1 == b_end) tk->strip_start[tk->n_strips] = tk->base + tk->emitted + tk->nl;   // the segment's last block: the tokens end HERE (what the
        }                                                                                          // counting passes saw behind it is not the image's)
        if (MODE == SUB_WRITE && done) {
            mz[b] = (uint8_t)(full ? 64 : z);                                    // m_mcu_block_max_zag :2512 (EOB: the position it was read at)
            if (!inherited) {
                uint4* src = reinterpret_cast<uint4*>(blk);
                uint4* dst = reinterpret_cast<uint4*>(out + b * 64);             // 128-byte blocks at 128-byte-aligned offsets (checked by the host)
                #pragma unroll
                for (int i = 0; i < 8; ++i) { dst[i] = src[i]; src[i] = make_uint4(0, 0, 0, 0); }
            }
            inherited = false;
        }
        if (MODE == SUB_FIRST && done) break;                                    // the inherited block is complete
        b += done ? 1 : 0; nblk += done ? 1 : 0;
        z = done ? 0 : znew;
        c = done ? (c + 1 == x.nb ? 0 : c + 1) : c;
        if (MODE == SUB_TOKENS && (++steps & 15u) == 0) tk->flush();             // every lane of the wave at once: at most 16 tokens wait
        if (MODE == SUB_COUNT && br.pos >= ck_next) {                            // (never true without a trace)
            while (ck_j < tr->n_ck && br.pos >= ck_next) {                         // one symbol may step over several checkpoints (tiny steps)
                SubCk& k = tr->ck[ck_j];
                const uint16_t cz = (uint16_t)(c | z << 4);
                if (tr->compare && k.pos == br.pos && k.cz == cz) {              // in step with the previous pass from here on
                    // what this pass counted up to here instead of the previous one: the later checkpoints and the totals move by it
                    const int dn = (int16_t)((uint16_t)nblk - k.nblk), dt = (int16_t)((uint16_t)ntok - k.ntok);
                    const int e0 = (int16_t)((uint16_t)dc0 - (uint16_t)k.dcs[0]), e1 = (int16_t)((uint16_t)dc1 - (uint16_t)k.dcs[1]), e2 = (int16_t)((uint16_t)dc2 - (uint16_t)k.dcs[2]);
                    for (int jj = ck_j; jj < tr->n_ck; ++jj) {
                        SubCk& q = tr->ck[jj];
                        q.nblk = (uint16_t)(q.nblk + dn); q.ntok = (uint16_t)(q.ntok + dt);
                        q.dcs[0] = (int16_t)(q.dcs[0] + e0); q.dcs[1] = (int16_t)(q.dcs[1] + e1); q.dcs[2] = (int16_t)(q.dcs[2] + e2);
                    }
                    nblk = tr->old_nblk + dn; ntok = tr->old_ntok + dt; dc0 = tr->old_dcs[0] + e0; dc1 = tr->old_dcs[1] + e1; dc2 = tr->old_dcs[2] + e2;
                    tr->stopped = true; tr->stop_ck = ck_j;
                    break;
                }
                k.pos = br.pos; k.cz = cz; k.nblk = (uint16_t)nblk; k.ntok = (uint16_t)ntok; k.dcs[0] = (int16_t)dc0; k.dcs[1] = (int16_t)dc1; k.dcs[2] = (int16_t)dc2;
                ++ck_j; ck_next += tr->step_bits;
            }
            if (tr->stopped) break;
            if (ck_j == tr->n_ck) ck_next = 0xFFFFFFFFu;
        }
    }
    if (MODE == SUB_COUNT && tr) tr->ntok = ntok;
    // A pass that ran to its end leaves no checkpoint of an EARLIER pass standing: one that lies in the few bits a pass may overshoot its
    // sub-sequence by is reached by some passes and not by others, and a later pass that matched it would add its difference to the totals
    // of the pass before it -- which never stood there.  (Found in round 4 with nine checkpoints per lane, i.e. closer ones: the last block of
    // a restart segment lost; six had passed every test and 1 000 fuzzed files.)
    if (MODE == SUB_COUNT && tr && !tr->stopped) for (int jj = ck_j; jj < tr->n_ck; ++jj) tr->ck[jj].pos = 0xFFFFFFFFu;
    if (MODE == SUB_COUNT && tr && tr->stopped) { dcs[0] = dc0; dcs[1] = dc1; dcs[2] = dc2; return ok; }      // s: untouched, the caller keeps the previous exit state
    if (MODE == SUB_TOKENS) tk->flush();
    if (MODE == SUB_WRITE && z > 0 && !inherited && b < b_end) {                 // a block of this lane's that the next lanes finish: its line, as far as it goes
        const uint4* src = reinterpret_cast<const uint4*>(blk);
        uint4* dst = reinterpret_cast<uint4*>(out + b * 64);
        #pragma unroll
        for (int i = 0; i < 8; ++i) dst[i] = src[i];
    }
    dcs[0] = dc0; dcs[1] = dc1; dcs[2] = dc2;
    s.pos = br.pos; s.c = (uint16_t)c; s.z = (uint16_t)z;
    return ok;
}

// NH: Huffman / quantisation tables kept in LDS (0 = none: read from global memory).  A batch written by one encoder has four
// Huffman tables; with room for four instead of eight a workgroup needs 47 KB instead of 58, and a compute unit holds three of
// them instead of two -- the kernel is a chain of dependent operations per lane, what it lacks is waves to alternate with.
#ifndef JPEG_SYNC_PROFILE           // measurement only (tools/variant.sh jpeg_host:jprof:-DJPEG_SYNC_PROFILE=1, tools/jpeg_sync_prof.py): cycles per phase, thread 0's clock
#define JPEG_SYNC_PROFILE 0
#endif
#if JPEG_SYNC_PROFILE
__device__ unsigned long long g_sync_prof[16];      // 0-4 cycles per phase, 6 re-decode sweeps, 7 segments; 8 lanes that decoded again, 9 of them
                                                     // stopped at a checkpoint, 10 the sum of those checkpoints' numbers, 11 ran to the end of their sub-sequence,
                                                     // 12 of those: left in another state than before (the lane behind must decode again)
#define SPROF_DECL unsigned long long sp_t0 = clock64()
#define SPROF(slot) do { const unsigned long long now_ = clock64(); if (threadIdx.x == 0) atomicAdd(&g_sync_prof[slot], now_ - sp_t0); sp_t0 = now_; } while (0)
#define SPROF_COUNT(slot, n) do { if (threadIdx.x == 0) atomicAdd(&g_sync_prof[slot], (unsigned long long)(n)); } while (0)
#define SPROF_LANE(slot, n) atomicAdd(&g_sync_prof[slot], (unsigned long long)(n))
#else
#define SPROF_DECL
#define SPROF(slot)
#define SPROF_COUNT(slot, n)
#define SPROF_LANE(slot, n)
#endif
template <int NH, bool TOK = false>
__global__ __launch_bounds__(kSyncThreads) void k_jpeg_entropy_sync(const DevItem* items, const DevImage* images,
                                                                    const DevHuff* huff_g, int n_huff, const int16_t* quant_g, int n_quant,
                                                                    const uint8_t* blob, int16_t* coeffs, uint8_t* max_zag, uint32_t* status,
                                                                    uint32_t* tokens = nullptr, uint32_t* strip_tab = nullptr, int n_ck_arg = 0)
{
    constexpr bool IN_LDS = NH > 0;
    __shared__ DevHuff sh_huff[IN_LDS ? NH : 1];
    __shared__ int16_t sh_quant[IN_LDS ? NH * 64 : 1];
    __shared__ uint8_t sh_zag[64];
    __shared__ SubState exit_state[kSyncThreads];
    __shared__ int changed, failed, par[9];
    constexpr int kPitch = TOK ? 80 : 144, kSubCkDefault = TOK ? 5 : 6;                     // a lane's piece of the staging area; its checkpoints (up to kPitch / 16:
    const int kSubCk = n_ck_arg > 0 && n_ck_arg <= kPitch / (int)sizeof(SubCk) ? n_ck_arg : kSubCkDefault;    // GAMUT_HIP_JPEG_CHECKPOINTS, tests)             // a lane's piece of the staging area; its checkpoints
    __shared__ __attribute__((aligned(16))) uint8_t sh_blk[kSyncThreads * kPitch];          // the write sweep: a block per lane (144-byte pitch) / 16 tokens
    // blocks finished, DC-difference sums of the three components, tokens: prefix-summed between the counting passes and the write sweep,
    // in the staging area (whose checkpoints are done with by then, and which is cleared afterwards)
    int (*scan)[kSyncThreads] = reinterpret_cast<int (*)[kSyncThreads]>(sh_blk);
    static_assert(5 * kSyncThreads * sizeof(int) <= kSyncThreads * kPitch && kPitch / (int)sizeof(SubCk) <= kSubCkMax && kPitch % 16 == 0 && kPitch >= 64, "the scan, the checkpoints and 16 tokens borrow the staging area");
    load_tables<IN_LDS, kSyncThreads>(sh_huff, sh_quant, sh_zag, huff_g, n_huff, quant_g, n_quant);
    const int t = threadIdx.x;
    {
        uint4* zb = reinterpret_cast<uint4*>(sh_blk + t * kPitch);
        #pragma unroll
        for (int i = 0; i < kPitch / 16; ++i) zb[i] = make_uint4(0, 0, 0, 0);
    }
    SPROF_DECL;
    const DevItem it = items[blockIdx.x];
    const DevImage im = images[it.image];
    if (t == 0) {
        changed = 0; failed = 0;
        par[0] = im.quant[0]; par[1] = im.quant[1]; par[2] = im.quant[2]; par[3] = im.dc[0]; par[4] = im.dc[1]; par[5] = im.dc[2];
        par[6] = im.ac[0]; par[7] = im.ac[1]; par[8] = im.ac[2];
    }
    __syncthreads();
    const uint32_t len = (uint32_t)(it.end - it.begin);
    const uint32_t sub = max(64u, ((len + kSyncThreads - 1) / kSyncThreads + 3) & ~3u);     // bytes per lane
    const int nsub = (int)((len + sub - 1) / sub);
    const bool active = t < nsub;
    const SubCtx x{ IN_LDS ? sh_huff : huff_g, IN_LDS ? sh_quant : quant_g, sh_zag, blob + it.begin, min((uint32_t)(t + 1) * sub, len) * 8u,
                    par, (uint32_t)im.org, im.nb };
    int16_t* out = TOK ? nullptr : coeffs + im.coeff_off + (int64_t)it.first_mcu * im.nb * 64;
    uint8_t* mz = max_zag + im.zag_off + (int64_t)it.first_mcu * im.nb;
    const int64_t total_blocks = (int64_t)it.n_mcus * im.nb;

    // sweep 0: every lane from the start of its own sub-sequence, as if a block began there
    SubState entry{ (uint32_t)t * sub * 8u, 0, 0 }, mine = entry;
    int nblk = 0, dcs[3] = { 0, 0, 0 }, ntok = 0;
    SubTrace tr;
    tr.ck = reinterpret_cast<SubCk*>(sh_blk + t * kPitch); tr.n_ck = kSubCk; tr.first_bit = (uint32_t)t * sub * 8u; tr.step_bits = ((sub + (uint32_t)kSubCk) / (uint32_t)(kSubCk + 1)) * 8u;
    tr.compare = false; tr.old_nblk = 0; tr.old_dcs[0] = tr.old_dcs[1] = tr.old_dcs[2] = 0; tr.old_ntok = 0; tr.ntok = 0; tr.stopped = false;
    if (active) {
        for (int j = 0; j < kSubCk; ++j) tr.ck[j].pos = 0xFFFFFFFFu;             // (a pass that ends early leaves the later ones unset: never a match)
        sub_decode<SUB_COUNT>(x, mine, nblk, dcs, 0, 0, nullptr, nullptr, nullptr, &tr);
        ntok = tr.ntok;
    }
    exit_state[t] = mine;
    __syncthreads();
    SPROF(0);
    // sweeps 1..: from the predecessor's exit state, until nothing moves
    bool settled = false;
    for (int sweep = 0; sweep < kSyncThreads + 1; ++sweep) {
        SubState from = t == 0 ? SubState{ 0, 0, 0 } : exit_state[t - 1];
        __syncthreads();                                        // everybody has read its predecessor
        if (active && (sweep == 0 || !same(from, entry))) {
            entry = from; mine = from;
            tr.compare = true; tr.old_nblk = nblk; tr.old_dcs[0] = dcs[0]; tr.old_dcs[1] = dcs[1]; tr.old_dcs[2] = dcs[2]; tr.old_ntok = ntok;
            dcs[0] = dcs[1] = dcs[2] = 0;
            sub_decode<SUB_COUNT>(x, mine, nblk, dcs, 0, 0, nullptr, nullptr, nullptr, &tr);
            ntok = tr.ntok;
            SPROF_LANE(8, 1); if (tr.stopped) { SPROF_LANE(9, 1); SPROF_LANE(10, tr.stop_ck); } else { SPROF_LANE(11, 1); if (!same(mine, exit_state[t])) SPROF_LANE(12, 1); }
            if (!tr.stopped && !same(mine, exit_state[t])) { exit_state[t] = mine; changed = 1; }
        }
        __syncthreads();
        const int any = changed;
        __syncthreads();
        if (t == 0) changed = 0;
        SPROF_COUNT(6, 1);
        if (!any) { settled = true; break; }
    }
    SPROF(1);
    (void)settled;                                              // the loop bound (one lane settles per sweep at worst) always reaches the fixed point
    // exclusive prefix sums over the lanes: first block, DC predictors and first token of every lane
    scan[0][t] = active ? nblk : 0; scan[1][t] = active ? dcs[0] : 0; scan[2][t] = active ? dcs[1] : 0; scan[3][t] = active ? dcs[2] : 0;
    scan[4][t] = active ? ntok : 0;
    __syncthreads();
    for (int d = 1; d < kSyncThreads; d <<= 1) {
        int v[5];
        #pragma unroll
        for (int k = 0; k < 5; ++k) v[k] = t >= d ? scan[k][t - d] : 0;
        __syncthreads();
        #pragma unroll
        for (int k = 0; k < 5; ++k) scan[k][t] += v[k];
        __syncthreads();
    }
    const int64_t b0 = active ? scan[0][t] - nblk : 0;
    const int pred_in[3] = { scan[1][t] - dcs[0], scan[2][t] - dcs[1], scan[3][t] - dcs[2] };
    const int64_t finished = scan[0][kSyncThreads - 1];
    const uint32_t tok0 = (uint32_t)(scan[4][t] - ntok), tok_total = (uint32_t)scan[4][kSyncThreads - 1];
    __syncthreads();                                            // everybody has its prefix sums: the area is the staging area again
    SPROF(2);
    {                                                           // the checkpoints are done with: the staging area starts out zero
        uint4* zb = reinterpret_cast<uint4*>(sh_blk + t * kPitch);
        #pragma unroll
        for (int i = 0; i < kPitch / 16; ++i) zb[i] = make_uint4(0, 0, 0, 0);
    }
    if constexpr (TOK) {
        // the compact hand-off: tokens instead of blocks (sub_decode<SUB_TOKENS>).  A stream that would emit more tokens than the image's
        // slot holds (only a damaged one can: the slot is sized from the scan's length) emits none and is flagged.
        uint32_t* const strip_start = strip_tab + im.strip_off;
        const bool fits = tok_total <= (uint32_t)im.tok_cap;
        if (!fits && t == 0) failed = 1;
        if (active && fits) {
            int pred[3] = { pred_in[0], pred_in[1], pred_in[2] };
            SubState s = entry; int n2 = 0;
            TokCtx tk;
            tk.out = tokens + im.tok_off + tok0; tk.lds = reinterpret_cast<uint32_t*>(sh_blk + t * kPitch); tk.strip_start = strip_start;
            tk.base = tok0; tk.total = (uint32_t)ntok; tk.emitted = 0; tk.nl = 0;
            tk.SB = im.sb; tk.row_blocks = im.row_blocks; tk.n_strips = (uint32_t)im.n_strips;
            const int64_t gb = (int64_t)it.first_mcu * im.nb + b0;               // the lane's first block, in the image
            const int64_t row = gb / im.row_blocks; const int local = (int)(gb - row * im.row_blocks);
            const int strips_per_row = (im.row_blocks + im.sb - 1) / im.sb;
            tk.strip = (uint32_t)(row * strips_per_row + local / im.sb); tk.sb = local % im.sb; tk.left_in_row = im.row_blocks - local;
            if (!sub_decode<SUB_TOKENS>(x, s, n2, pred, b0, total_blocks, nullptr, mz, nullptr, nullptr, &tk)) failed = 1;
            if (t == nsub - 1 && b0 + n2 < total_blocks) failed = 1;      // the segment ended before its last block did (behind it: not this interval's)
            if (it.tail >= 0 && b0 < total_blocks && b0 + n2 == total_blocks && restart_leftover_bad(x.seg, len, s.pos, it.tail)) atomicOr(status + it.image, kStatusBadRestart);   // the lane that ended the last block
        }
        __syncthreads();
        // the strips no block opened (a damaged stream ends early) are empty: their tokens "begin" at the end; blocks nobody reached
        // have no coefficients (their strips' tiles stay zero) and max_zag 1
        int64_t started = fits ? finished + (exit_state[nsub > 0 ? nsub - 1 : 0].z > 0 ? 1 : 0) : 0;
        started = started > total_blocks ? total_blocks : started;
        const int strips_per_row = (im.row_blocks + im.sb - 1) / im.sb;
        int64_t first_empty = 0;
        if (started > 0) { const int64_t lb = started - 1, row = lb / im.row_blocks; first_empty = row * strips_per_row + (lb - row * im.row_blocks) / im.sb + 1; }
        const uint32_t end_tok = fits ? tok_total : 0u;
        const bool complete = fits && finished >= total_blocks;                   // the lane that finished the last block wrote the end of the tokens itself
        for (int64_t sidx = first_empty + t; sidx < im.n_strips + (complete ? 0 : 1); sidx += kSyncThreads) strip_start[sidx] = end_tok;
        for (int64_t blk = started + t; blk < total_blocks; blk += kSyncThreads) mz[blk] = 1;
        SPROF(3);
        SPROF(4);
        SPROF_COUNT(7, 1);
        if (t == 0 && failed) atomicOr(status + it.image, 1u);
        return;
    }
    if (active) {
        int pred[3] = { pred_in[0], pred_in[1], pred_in[2] };
        SubState s = entry; int n2 = 0;
        if (!sub_decode<SUB_WRITE>(x, s, n2, pred, b0, total_blocks, out, mz, reinterpret_cast<int16_t*>(sh_blk + t * kPitch))) failed = 1;
        if (t == nsub - 1 && b0 + n2 < total_blocks) failed = 1;      // the segment ended before its last block did (behind it: not this interval's)
        if (it.tail >= 0 && b0 < total_blocks && b0 + n2 == total_blocks && restart_leftover_bad(x.seg, len, s.pos, it.tail)) atomicOr(status + it.image, kStatusBadRestart);       // the lane that ended the last block
    }
    __threadfence();                                            // the lines are on their way before anybody adds single coefficients to them
    __syncthreads();
    SPROF(3);
    if (active && entry.z > 0 && b0 < total_blocks) {           // the rest of the block this lane found half-decoded
        int pred[3] = { 0, 0, 0 }; SubState s = entry; int n3 = 0;
        sub_decode<SUB_FIRST>(x, s, n3, pred, b0, total_blocks, out, mz);
    }
    // A segment whose decode ended early (damaged data) leaves blocks nobody started: they are cleared, not left as they were
    const int64_t started = finished + (exit_state[nsub > 0 ? nsub - 1 : 0].z > 0 ? 1 : 0);
    for (int64_t blk = started + t; blk < total_blocks; blk += kSyncThreads) {
        uint4* dst = reinterpret_cast<uint4*>(out + blk * 64);
        #pragma unroll
        for (int i = 0; i < 8; ++i) dst[i] = make_uint4(0, 0, 0, 0);
    }
    __syncthreads();
    SPROF(4);
    SPROF_COUNT(7, 1);
    if (t == 0 && failed) atomicOr(status + it.image, 1u);
}

// ---- the scan as it stands in the file -> the unstuffed, padded segments the two kernels above read, ON THE DEVICE --------------------
// get_bits_no_markers (jpegload.d:722-743) and get_octet (:683-696) skip the 0x00 behind a data 0xFF while they read, and
// process_restart (:2335-2402) finds the RSTn markers; round 3 did both on host threads (unstuff_file below: memchr + many small
// memcpy into pinned memory, "unstuff + upload at 33 GB/s", and a thread pool that is divided by the ranks of the node).  Here the host
// copies the file's bytes from the first scan byte on into pinned memory as they are -- one memcpy -- and a workgroup per file turns them
// into the blob form: tiles of 4 KiB, a byte dropped when it is 0x00 behind 0xFF (prefix sum of the kept bytes over the workgroup,
// staged in LDS, written out as whole aligned 16-byte chunks); the data of a segment ends at the first 0xFF that is followed by
// anything but 0x00 (rare: a tile is processed up to the first such place and the marker handled by the whole workgroup in step) --
// an expected RSTn closes the segment (64 bytes of 0xFF behind it, as the host writes them) and opens the next, anything else ends the
// scan.  The segment list (image, first MCU, MCU count per restart interval) comes from the host, which knows it from the header;
// begin / end are filled in here.  A wrong or missing restart marker flags the file (status bit 3) and empties its segments.
struct DevRaw {
    uint64_t raw_begin, raw_len;        // the file from its first scan byte to its end, in the raw blob
    uint64_t out_begin, out_cap;        // the file's slot in the unstuffed blob (16-byte aligned)
    int32_t  image, first_item, n_items, restart_interval;
};
constexpr int kUnstuffThreads = 256, kUnstuffTile = kUnstuffThreads * 16;
__global__ __launch_bounds__(kUnstuffThreads) void k_jpeg_unstuff(const DevRaw* files, DevItem* items, const uint8_t* raw, uint8_t* blob, uint32_t* status,
                                                                   uint32_t* scan_end /* [image]: bytes from the scan's first byte to the marker that ends it (find_eoi starts there) */)
{
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    struct __attribute__((packed, aligned(1))) AnyVec { u32x4 v; };
    __shared__ __attribute__((aligned(16))) uint8_t stage[16 + kUnstuffTile + 64 + 16];
    __shared__ uint32_t wave_sum[kUnstuffThreads / 64];
    __shared__ uint32_t first_term;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const DevRaw f = files[blockIdx.x];
    const uint8_t* src = raw + f.raw_begin;
    uint8_t* const dst = blob + f.out_begin;
    uint64_t cur = 0, w = 0, seg_begin = 0;                 // next raw byte; bytes produced (the last w % 16 of them still in stage[])
    uint32_t carry = 0;
    int seg = 0, expect = 0;
    bool bad = false;
    // stage[0 .. m) = the last m of the w bytes produced -> dst, whole 16-byte chunks; the rest moves to the front (all threads call it)
    auto flush = [&](uint32_t m) {
        __syncthreads();
        const uint32_t chunks = m >> 4;
        const uint64_t base = w - m;                         // 16-byte aligned by construction
        for (uint32_t c = t; c < chunks; c += kUnstuffThreads) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(stage + c * 16);
            if (base + c * 16 + 16 <= f.out_cap) *reinterpret_cast<u32x4*>(dst + base + c * 16) = v;
        }
        uint8_t keep = 0;
        const uint32_t rest = m & 15u;
        if ((uint32_t)t < rest) keep = stage[chunks * 16 + t];
        __syncthreads();
        if ((uint32_t)t < rest) stage[t] = keep;
        __syncthreads();
        return rest;
    };
    auto close_segment = [&](int tail) {                     // the segment's item, then its 64 bytes of padding; tail: DevItem.tail
        if (t == 0 && seg < f.n_items) { items[f.first_item + seg].begin = f.out_begin + seg_begin; items[f.first_item + seg].end = f.out_begin + w; items[f.first_item + seg].tail = tail; }
        if (t < 64) stage[carry + t] = 0xFF;
        const uint32_t m = carry + 64;
        w += 64;
        carry = flush(m);
        seg_begin = w; ++seg;
    };
    bool ended = false;
    while (!ended) {
        const uint64_t left = f.raw_len - cur;
        const uint32_t n = left < (uint64_t)kUnstuffTile ? (uint32_t)left : (uint32_t)kUnstuffTile;
        if (t == 0) first_term = 0xFFFFFFFFu;
        __syncthreads();
        // this thread's 16 bytes, the byte in front of them and the byte behind them (zeros outside the data)
        const uint32_t o = (uint32_t)t * 16u;
        uint8_t b[18];
        #pragma unroll
        for (int k = 0; k < 18; ++k) b[k] = 0;
        if (o < n) {
            const u32x4 v = reinterpret_cast<const AnyVec*>(src + cur + o)->v;          // (the raw blob has 32 bytes of slack behind every file)
            #pragma unroll
            for (int k = 0; k < 16; ++k) b[1 + k] = (uint8_t)(v[k >> 2] >> ((k & 3) * 8));
            b[0] = cur + o > 0 ? src[cur + o - 1] : 0;
            b[17] = src[cur + o + 16];
        }
        uint32_t term = 0xFFFFFFFFu;
        #pragma unroll
        for (int k = 15; k >= 0; --k) {
            const uint64_t at = cur + o + (uint32_t)k;
            if (o + (uint32_t)k < n && b[1 + k] == 0xFF && at + 1 < f.raw_len && b[2 + k] != 0x00) term = o + (uint32_t)k;
        }
        if (term != 0xFFFFFFFFu) atomicMin(&first_term, term);
        __syncthreads();
        const uint32_t p = first_term;                       // offset of the first data-ending 0xFF in the tile, if any
        const uint32_t region = p < n ? p : n;
        // kept bytes of [0, region): everything but a 0x00 behind a 0xFF
        uint32_t cnt = 0, keepmask = 0;
        #pragma unroll
        for (int k = 0; k < 16; ++k) {
            const bool keep = o + (uint32_t)k < region && !(b[1 + k] == 0x00 && b[k] == 0xFF);
            keepmask |= keep ? 1u << k : 0u; cnt += keep ? 1u : 0u;
        }
        uint32_t incl = cnt;                                 // inclusive prefix sum over the wave, then over the workgroup
        #pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t up = __shfl_up(incl, d, 64); if (lane >= d) incl += up; }
        if (lane == 63) wave_sum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        #pragma unroll
        for (int k = 0; k < kUnstuffThreads / 64; ++k) { const uint32_t s = wave_sum[k]; before += k < wave ? s : 0u; total += s; }
        const uint32_t at = carry + before + incl - cnt;
        if (cnt == 16) {
            u32x4 v;
            #pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (uint32_t)b[1 + 4 * k] | (uint32_t)b[2 + 4 * k] << 8 | (uint32_t)b[3 + 4 * k] << 16 | (uint32_t)b[4 + 4 * k] << 24;
            reinterpret_cast<AnyVec*>(stage + at)->v = v;                               // (LDS takes byte-unaligned 16-byte accesses on gfx950)
        } else if (cnt) {
            uint32_t q = at;
            #pragma unroll
            for (int k = 0; k < 16; ++k) if (keepmask >> k & 1u) stage[q++] = b[1 + k];
        }
        w += total;
        carry = flush(carry + total);
        if (p < n) {                                         // a marker: skip fill bytes, look at its code (every thread reads the same bytes)
            uint64_t j = cur + p + 1;
            while (j < f.raw_len && src[j] == 0xFF) ++j;
            const uint32_t code = j < f.raw_len ? src[j] : 0xD9u;
            const bool rst = code >= 0xD0u && code <= 0xD7u && f.restart_interval > 0 && seg + 1 < f.n_items;
            if (rst && code != 0xD0u + (uint32_t)expect) { bad = true; ended = true; }
            else if (rst) { close_segment((int)min(j - (cur + p + 1), (uint64_t)4096)); expect = (expect + 1) & 7; cur = j + 1; }
            else { ended = true; if (t == 0) scan_end[f.image] = (uint32_t)(cur + p); }      // EOI or any other marker ends the scan
        } else {
            cur += n;
            if (cur >= f.raw_len) { ended = true; if (t == 0) scan_end[f.image] = (uint32_t)f.raw_len; }   // the file ends inside the scan: what is there is the data
        }
    }
    if (!bad) {
        if (seg + 1 == f.n_items) close_segment(-1);
        else bad = true;                                     // a restart marker is missing
    }
    if (carry) {                                             // the last, partial chunk (the slot has room for a whole one)
        __syncthreads();
        if (t == 0 && (w - carry) + 16 <= f.out_cap) *reinterpret_cast<u32x4*>(dst + (w - carry)) = *reinterpret_cast<const u32x4*>(stage);
    }
    if (bad) {
        for (int k = t; k < f.n_items; k += kUnstuffThreads) { items[f.first_item + k].begin = f.out_begin; items[f.first_item + k].end = f.out_begin; }
        if (t == 0) atomicOr(status + f.image, kStatusBadRestart);
    }
}
