// jpeg_batch.hpp -- batch orchestration of the baseline device entropy decode.  Included by jpeg_host.hip inside its namespace, behind
// jpeg_parse.hpp (the marker parser) and jpeg_entropy_kernels.hpp (the device structs and kernels), in front of jpeg_prog.hpp (which
// shares the helpers at the top of this file; the stream guard and the trace clock are common.hpp's).
//
// Host side: header walk per file (on host threads), table de-duplication, restart-interval index, uploads per group of files and the
// groups' kernels; entropy_decode_device at the end of the file is the list of the stages.

// host threads of a batch stage: host_threads() within 1..16, and no more than `cap` (the work there is)
inline int batch_workers(int cap)
{
    int workers = host_threads();
    workers = workers < 1 ? 1 : workers > 16 ? 16 : workers;
    return workers > cap ? cap : workers;
}
// a Parser per worker of a parallel_for (a Parser is 10 KB of tables: not on a worker's stack)
struct ParserPool {
    std::vector<std::unique_ptr<Parser>> parsers;
    explicit ParserPool(int workers) { for (int w = 0; w < workers; ++w) parsers.emplace_back(new Parser()); }
    Parser& operator[](int w) { return *parsers[(size_t)w]; }
};
template <class T> int intern(std::vector<T>& pool, const T& t)      // index of a bit-identical table, appended if new
{
    for (size_t i = 0; i < pool.size(); ++i) if (!memcmp(&pool[i], &t, sizeof(T))) return (int)i;
    pool.push_back(t);
    return (int)pool.size() - 1;
}
struct QuantTab { int16_t q[64]; };
// a DevHuff is a function of the code-length counts and the symbols (to_dev_huff): maxcode[] / delta[] hold the former, vals[] the latter -- 396 bytes
// decide whether two tables are the same one, not 2048 (the serial de-duplication walks six tables of every file of a batch)
inline int intern(std::vector<DevHuff>& pool, const DevHuff& t)
{
    static_assert(offsetof(DevHuff, vals) + sizeof(t.vals) - offsetof(DevHuff, maxcode) == sizeof(t.maxcode) + sizeof(t.delta) + sizeof(t.vals), "DevHuff: maxcode, delta, vals adjacent");
    const size_t from = offsetof(DevHuff, maxcode), n = sizeof(t.maxcode) + sizeof(t.delta) + sizeof(t.vals);
    for (size_t i = 0; i < pool.size(); ++i) if (!memcmp((const char*)&pool[i] + from, (const char*)&t + from, n)) return (int)i;
    pool.push_back(t);
    return (int)pool.size() - 1;
}

// What the host prepares for one file, independently of every other file (so files are spread over host threads), in two
// steps: (A) header walk + tables in device form + an upper bound of the file's share of the upload; (C) the entropy-coded
// segments copied UNSTUFFED (the 0x00 after a data 0xFF dropped) straight into the pinned upload image, cut at the RSTn
// markers, each followed by 64 bytes of 0xFF.
struct FilePrep {
    int rc = GAMUT_HIP_OK; char msg[200] = { 0 };
    bool progressive = false;                                  // SOF2: left to progressive_decode_device (rc = kDeferred)
    int comps = 0, nb = 0, ny = 0; uint32_t org = 0;           // org: DevImage.org
    QuantTab quant[3];
    // [component][DC, AC]: six tables of 2 KB -- not inside the record: a vector of 1024 records was 13 MB that the constructor cleared on ONE thread
    // in front of everything else (most of the "headers" phase).  The batch call points them into one uninitialised block per thread that it keeps.
    DevHuff (*huff)[2] = nullptr;
    size_t scan_pos = 0, cap = 0, used = 0;                    // first scan byte in the file; bound / actual size of the unstuffed segments
    int restart_interval = 0, total_mcus = 0;
    bool dev_unstuff = false;                                  // the scan goes up as it is and k_jpeg_unstuff makes the segments (items: begin / end filled in there)
    size_t raw_len = 0;                                        // bytes from scan_pos to the end of the file
    size_t scan_end = 0;                                       // host-unstuffed files: where the scan's data ended (the marker find_eoi starts at), from the start of the file
    std::vector<DevItem> items;                                // begin / end relative to the file's slot in the blob; pad = (estimated) bytes of the segment
};
// FilePrep.rc of a file the host feeder decodes after the device pass: not for the kernels (prepare_header), a restart structure the unstuffing could
// not follow, or anything a kernel flagged -- a bit pattern no code word begins, a segment that ran out, octets left in front of a marker.  The
// reference has a result for many of those (jpgd decodes symbol 0 and carries on); the host feeder is the part of the library that knows them all.
constexpr int kHostRedo = -1001;
// where the 0x00 stuffing is dropped and the restart markers are found: GAMUT_HIP_JPEG_UNSTUFF=host / device forces either (tests, measurements)
int unstuff_site() { const char* e = getenv("GAMUT_HIP_JPEG_UNSTUFF"); return !e || !*e ? 0 : !strcmp(e, "host") ? 1 : !strcmp(e, "device") ? 2 : 0; }

// tests: GAMUT_HIP_JPEG_HOST_REDO=0 leaves a file an entropy KERNEL flagged refused (k_jpeg_entropy, k_jpeg_entropy_sync, k_jpeg_unstuff, k_prog_scan) -- the
// host feeder behind the device pass would hide a kernel that flags a stream it should have decoded (the result is right either way, only slower).  It
// covers the kernels' flags only: a file the HOST routes to the feeder before any kernel sees it (prepare_header: a scan header in the padding, a DC
// category above 15; unstuff_file: a restart structure it cannot follow; the progressive preparation likewise) is decoded there as ever.
inline bool redo_flagged_files() { const char* e = getenv("GAMUT_HIP_JPEG_HOST_REDO"); return !(e && *e && atoi(e) == 0); }

void prepare_header(int i, const uint8_t* base, size_t n, gamut_hip_jpeg_frame& f, FilePrep& out, Parser& P)
{
    P = Parser();
    out.rc = parse_baseline(P, base, n, &f, true);
    out.progressive = out.rc == GAMUT_HIP_ERR_UNSUPPORTED && P.progressive;
    if (out.rc != GAMUT_HIP_OK) { snprintf(out.msg, sizeof(out.msg), "image %d: %s", i, last_error_buf()); return; }
    // Files the kernels are not given (the host feeder decodes them behind the device pass, host_redo): a scan header that ends in the padding behind
    // the file (the scan's data is what the padding holds), a DC table with a category above 15 (the kernels mask it, the reference leaves its tables)
    if (P.pos >= n) { out.rc = kHostRedo; return; }
    for (int k = 0; k < P.scan.ncomp; ++k) if (P.huff[P.td[P.scan.comp[k]]].dc_limit > 15) { out.rc = kHostRedo; return; }
    out.comps = f.comps; out.nb = f.blocks_per_mcu; out.ny = f.comps == 1 ? 1 : P.hs[0] * P.vs[0];
    { int order[6] = { 0, 0, 0, 0, 0, 0 }; const int blocks = scan_block_order(P, order, 6); out.org = 0; for (int b = 0; b < blocks && b < 6; ++b) out.org |= (uint32_t)order[b] << (2 * b); }
    for (int c = 0; c < f.comps; ++c) {
        memcpy(out.quant[c].q, P.quant[P.tq[c]], sizeof(out.quant[c].q));
        for (int k = 0; k < 2; ++k) {
            to_dev_huff(P.huff[k ? P.ta[c] : P.td[c]], out.huff[c][k]);
        }
    }
    out.scan_pos = P.pos; out.restart_interval = P.restart_interval; out.total_mcus = f.mcus_per_row * f.mcus_per_col;
    // unstuffing only drops bytes; every segment (at most one per restart interval) gains 64 bytes of padding
    const size_t segs = out.restart_interval ? (size_t)(out.total_mcus / out.restart_interval + 1) : 1;
    out.cap = (n - out.scan_pos) + 64 * segs + 16;
    out.raw_len = n - out.scan_pos;
    // On the device unless the restart intervals are tiny (the kernel handles a marker by the whole workgroup in step: a file of
    // thousands of 30-byte intervals is quicker through memchr on a host thread; its segments take a lane each anyway)
    const size_t n_seg = out.restart_interval ? (size_t)((out.total_mcus + out.restart_interval - 1) / out.restart_interval) : 1;
    const size_t est = n_seg ? out.raw_len / n_seg : out.raw_len;
    out.dev_unstuff = unstuff_site() == 2 || (unstuff_site() == 0 && (out.restart_interval == 0 || est >= 1024));
    if (out.dev_unstuff) {
        out.items.resize(n_seg);
        for (size_t k = 0; k < n_seg; ++k) {
            DevItem& it = out.items[k]; memset(&it, 0, sizeof(it));
            it.image = i; it.first_mcu = out.restart_interval ? (int)k * out.restart_interval : 0;
            it.n_mcus = out.restart_interval ? std::min(out.restart_interval, out.total_mcus - it.first_mcu) : out.total_mcus;
            it.pad = (int32_t)std::min<size_t>(est, 0x7fffffff);
        }
        out.used = out.cap;
        // (Tried: scans of files that live in page-locked memory uploaded from where they are, a DMA per file -- 1024 x 225 kB: 17.0 ->
        // 20.1 ms, profiles/r04_pinned.txt: a DMA per file costs more than the copy into one pinned image and one DMA per group.  The QOI
        // call, whose files are megabytes, keeps that path: same time, no host copy.)
    }
}

// The marker walk both unstuffers share (the baseline one below, prog_unstuff in jpeg_prog.hpp): the entropy-coded bytes of ONE scan,
// base[begin, n), copied to dst + w without the 0x00 stuffing and cut at the RSTn markers the scan has a use for (`total` MCUs or
// units, `ri` of them per interval).  close(first, count, seg_begin, tail) records the segment dst[seg_begin, w) and appends its
// padding (false: no room in the slot).  `q_end` is where the walk stopped.  `n_is_scan_end`: the caller knows that the scan's data
// ends at n, so a marker that stops the walk sooner is an RSTn the scan has no use for.  Returns false for a restart structure that
// cannot be followed (what the reference makes of it is the host feeder's to say).
template <class Close>
bool unstuff_scan(const uint8_t* base, size_t begin, size_t n, int ri, int total, bool n_is_scan_end, uint8_t* dst, size_t cap, size_t& w, size_t& q_end, Close close)
{
    int next = 0, expect = 0;
    size_t q = begin, copy_from = begin, seg_begin = w;
    bool copying = true, bad = false;
    auto flush = [&](size_t upto) {
        if (copying && upto > copy_from) {
            const size_t k = upto - copy_from;
            if (w + k > cap) { bad = true; return; }                                       // cannot happen (see cap); never write past the slot
            memcpy(dst + w, base + copy_from, k); w += k;
        }
    };
    int fill = 0;                                          // 0xFF bytes in front of the marker under way, besides its own
    auto close_segment = [&](int count, int tail) {
        if (!close(next, count, seg_begin, tail)) { bad = true; return; }
        next += count; seg_begin = w;
    };
    while (!bad) {
        const uint8_t* hit = q < n ? (const uint8_t*)memchr(base + q, 0xFF, n - q) : nullptr;
        if (!hit || hit + 1 >= base + n) { flush(n); q = n; break; }
        const uint8_t m = hit[1];
        q = (size_t)(hit - base);
        if (m == 0x00) {
            if (!copying) { bad = true; break; }                                          // FF .. FF 00: the reference's input stopped at the FIRST of these FFs (not a stuffed byte: get_octet
            flush(q + 1); copy_from = q + 2; q += 2; continue;                            //  looks one byte ahead), process_restart then reads "FF, fill, 00": for the host feeder (kHostRedo)
        }                                                                                 // stuffed 0xFF: keep the FF, drop the 00
        flush(q); copying = false;                                                        // FF + non-zero: the data ends here (get_octet :683-696)
        if (m == 0xFF) { q += 1; fill = std::min(fill + 1, 4096); continue; }             // fill bytes before a marker
        if (m >= 0xD0 && m <= 0xD7 && ri && next + ri < total) {
            if (m != 0xD0 + expect) { bad = true; break; }
            close_segment(ri, fill); fill = 0;
            expect = (expect + 1) & 7; q += 2; copy_from = q; copying = true;
            continue;
        }
        break;                                             // EOI or any other marker ends the scan
    }
    if (!bad && n_is_scan_end && q < n) bad = true;
    if (!bad && next < total) {
        if (ri && total - next > ri) bad = true;           // a restart marker is missing
        else close_segment(total - next, -1);
    }
    q_end = q;
    return !bad;
}

void unstuff_file(int i, const uint8_t* base, size_t n, FilePrep& out, uint8_t* dst)
{
    size_t w = 0, q = 0;                                   // w = bytes written to dst
    const bool ok = unstuff_scan(base, out.scan_pos, n, out.restart_interval, out.total_mcus, false, dst, out.cap, w, q,
        [&](int first_mcu, int n_mcus, size_t seg_begin, int tail) {
            if (w + 64 > out.cap) return false;
            DevItem it{}; it.image = i; it.first_mcu = first_mcu; it.n_mcus = n_mcus; it.begin = seg_begin; it.end = w; it.tail = tail;
            it.pad = (int32_t)std::min<size_t>(w - seg_begin, 0x7fffffff);
            out.items.push_back(it);
            memset(dst + w, 0xFF, 64); w += 64;
            return true;
        });
    out.used = w; out.scan_end = q;
    if (!ok) { out.items.clear(); out.used = 0; out.rc = kHostRedo; }      // a wrong or missing RSTn: what the reference makes of it is the host feeder's to say
}

// The files of a batch the host feeder decodes (decode_coeffs, the whole of it: markers, scans, find_eoi): `deliver` takes the dense coefficients
// of a file that decoded; rcs[k] / msgs[k] receive the verdicts.  info[] gets the geometry and the density as the host feeder found them.
int host_redo(const uint8_t* const* data, const size_t* len, const std::vector<int>& idx, gamut_hip_jpeg_frame* info,
              const std::function<int(int i, const gamut_hip_jpeg_frame& fr)>& deliver, std::vector<int>& rcs, std::vector<std::string>& msgs)
{
    const int n = (int)idx.size();
    rcs.assign((size_t)n, GAMUT_HIP_OK); msgs.assign((size_t)n, std::string());
    if (!n) return GAMUT_HIP_OK;
    const int workers = batch_workers(n);
    // in chunks of `workers` files -- decode, deliver, free: a batch of a thousand damaged 4K files would otherwise hold their dense
    // coefficients (25 MB each) in host memory all at once
    int hip_rc = GAMUT_HIP_OK;
    std::vector<gamut_hip_jpeg_frame> frames((size_t)workers);
    for (int k0 = 0; k0 < n; k0 += workers) {
        const int m = std::min(workers, n - k0);
        for (int j = 0; j < m; ++j) memset(&frames[(size_t)j], 0, sizeof(gamut_hip_jpeg_frame));
        parallel_for(m, m, [&](int, int j) {
            const int k = k0 + j, i = idx[(size_t)k];
            rcs[(size_t)k] = decode_coeffs(data[i], len[i], &frames[(size_t)j]);
            if (rcs[(size_t)k] != GAMUT_HIP_OK) msgs[(size_t)k] = last_error_buf();
        });
        for (int j = 0; j < m; ++j) {
            const int k = k0 + j, i = idx[(size_t)k];
            gamut_hip_jpeg_frame& fr = frames[(size_t)j];
            if (rcs[(size_t)k] == GAMUT_HIP_OK && hip_rc == GAMUT_HIP_OK) hip_rc = deliver(i, fr);
            info[i] = fr; info[i].coeffs = nullptr; info[i].max_zag = nullptr;
            free(fr.coeffs); free(fr.max_zag); fr.coeffs = nullptr; fr.max_zag = nullptr;
        }
    }
    return hip_rc;
}
// ... into the caller's dense buffers (the coefficient-level entry point; progressive files at either level)
inline std::function<int(int, const gamut_hip_jpeg_frame&)> deliver_dense(const int64_t* coeff_offset, const int64_t* zag_offset, int16_t* d_coeffs, uint8_t* d_max_zag,
                                                                           uint32_t* d_status, hipStream_t stream)
{
    return [=](int i, const gamut_hip_jpeg_frame& fr) -> int {
        const size_t nblk = (size_t)fr.mcus_per_row * fr.mcus_per_col * fr.blocks_per_mcu;
        if (hipMemcpyAsync(d_coeffs + coeff_offset[i], fr.coeffs, nblk * 64 * sizeof(int16_t), hipMemcpyHostToDevice, stream) != hipSuccess ||
            hipMemcpyAsync(d_max_zag + zag_offset[i], fr.max_zag, nblk, hipMemcpyHostToDevice, stream) != hipSuccess ||
            (d_status && hipMemsetAsync(d_status + i, 0, sizeof(uint32_t), stream) != hipSuccess) ||
            hipStreamSynchronize(stream) != hipSuccess)          // (pageable sources, freed when host_redo returns)
            return set_error(GAMUT_HIP_ERR_HIP, "jpeg: upload of the coefficients of image %d failed", i);
        return GAMUT_HIP_OK;
    };
}

constexpr int kDeferred = -1000;                               // FilePrep.rc of a progressive file: not this function's business

// Hooks of the files -> pixels entry point (gamut_hip_jpeg_decode_batch_device): `layout` runs once the headers are known (it
// sizes and places the coefficient buffers: the caller of the coefficient-level entry point did that beforehand);
// `group_done(lo, hi, gs)` runs right after the entropy kernels of files [lo, hi) have been queued on stream gs -- the
// reconstruction of a group is queued behind its own entropy decode, beside the decode of the next group.
// The compact hand-off (tokens instead of dense blocks, SUB_TOKENS above) is the hook owner's choice per image: `tok_ok[i]` says which
// images could take it (4:2:0, one long segment, scan unstuffed on the device), `scan_len[i]` bounds their token count; the hook sets
// tok[i] and places the image's token slot and strip table (tok_off / strip_off / tok_cap; the buffers through d_tokens / d_strip_tab).
struct TokenPlan {
    const char* tok_ok; const size_t* scan_len;               // in
    char* tok; int64_t* tok_off; int64_t* strip_off; int32_t* tok_cap; uint32_t** d_tokens; uint32_t** d_strip_tab;     // out
};
struct DecodeHooks {
    std::function<int(const gamut_hip_jpeg_frame* info, const int* rc, const char* progressive, int64_t* coeff_offset, int64_t* zag_offset, int16_t** d_coeffs, uint8_t** d_max_zag,
                      const TokenPlan& plan)> layout;
    std::function<int(int lo, int hi, hipStream_t gs)> group_done;
    std::function<int(int i, const gamut_hip_jpeg_frame& fr, hipStream_t s)> redo;      // a file the host feeder decoded (host_redo): coefficients -> the hook owner's output
};

// the progressive files of a batch (jpeg_prog.hpp)
int progressive_decode_device(const uint8_t* const* data, const size_t* len, const std::vector<int>& idx,
                              const int64_t* coeff_offset, const int64_t* zag_offset,
                              int16_t* d_coeffs, uint8_t* d_max_zag, uint32_t* d_status,
                              gamut_hip_jpeg_frame* info, int* host_status, hipStream_t stream, int* first_index, char* first_msg, size_t msg_cap);

constexpr int kMaxGroups = 8;

// One call of entropy_decode_device: what its stages share.
// Pipeline: (A) headers on host threads -> (B) layout, and the coefficient clears go out on `stream` -> (C) segments
// unstuffed straight into the pinned upload image, slice by slice, each slice DMA'd on a private copy stream as soon as
// it is complete (so unstuffing, PCIe and the clears overlap) -> (D) tables, then the kernels on `stream` behind an event.
struct BaselineBatch {
    // the arguments (with hooks: the offsets and the coefficient buffers are the layout hook's to set)
    const uint8_t* const* data; const size_t* len; int count;
    const int64_t* coeff_offset; const int64_t* zag_offset;
    int16_t* d_coeffs; uint8_t* d_max_zag; uint32_t* d_status;
    gamut_hip_jpeg_frame* info; int* host_status; hipStream_t stream; const DecodeHooks* hooks;
    std::vector<int64_t> own_offsets;
    int workers = 1;
    // A. headers
    std::vector<FilePrep> prep;
    std::vector<int> progressive;                              // SOF2 files: decoded by progressive_decode_device after the baseline ones
    // the compact hand-off (TokenPlan), per image
    std::vector<char> tok; std::vector<int64_t> tok_off, strip_off; std::vector<int32_t> tok_cap;
    uint32_t* d_tokens = nullptr; uint32_t* d_strip_tab = nullptr;
    // B. tables, slots of the files in the blob and (files unstuffed on the device) in the raw image
    std::vector<DevImage> images; std::vector<DevHuff> huffs; std::vector<QuantTab> quants;
    std::vector<size_t> blob_off, raw_off;
    size_t blob_size = 0, raw_size = 0, max_items = 0; int n_dev_files = 0; bool any_ok = false;
    // staging: pinned and device images of the segments, the raw scans and the tables; status words
    uint8_t* d_blob = nullptr; uint8_t* h_blob = nullptr; uint8_t* d_raw = nullptr; uint8_t* h_raw = nullptr; uint8_t* d_tab = nullptr; uint8_t* h_tab = nullptr;
    uint32_t* st = nullptr; uint32_t* d_scan_end = nullptr;   // st: where the kernels flag errors (null: no device pass)
    size_t o_huff = 0, o_quant = 0, o_raws = 0, tab_total = 0, items_off = 0; int raws_done = 0;
    bool in_lds = false;
    // streams and events (the thread's own: the context only borrows them)
    hipStream_t copy_stream = nullptr; hipStream_t* side = nullptr; hipEvent_t* group_ready = nullptr; int n_groups = 1, n_lanes = 1;
    StreamDrain drain;
    // the group under way: its segment list (tokens | long | short), the files of it that are unstuffed on the device
    std::vector<DevItem> items; std::vector<DevRaw> raws; int n_tok = 0, n_long = 0;
    DevItem* d_items = nullptr; const DevRaw* d_raws = nullptr;
    // trace
    const bool trace = trace_enabled(); const TracePoint t_begin = trace_now(); TracePoint t_up;
    double ms_parse = 0, ms_upload = 0, ms_kernels_issue = 0; int total_long = 0, total_short = 0;

    const DevImage* d_img() const { return (const DevImage*)d_tab; }
    const DevHuff* d_huff() const { return (const DevHuff*)(d_tab + o_huff); }
    const int16_t* d_quant() const { return (const int16_t*)(d_tab + o_quant); }
    int n_huff() const { return (int)huffs.size(); }
    int n_quant() const { return (int)quants.size(); }
};

// A. the header walk of every file, on host threads
int prepare_headers(BaselineBatch& b)
{
    const int count = b.count;
    b.workers = batch_workers((count + 7) / 8);
    b.prep.resize((size_t)count);
    {
        struct FreeIt { void operator()(DevHuff* p) const { free(p); } };
        static thread_local std::unique_ptr<DevHuff, FreeIt> table_store; static thread_local size_t table_store_cap = 0;      // (kept by the thread, host memory only: warm pages,
        if ((size_t)count * 6 > table_store_cap) {                                                                              //  no clearing; every table is written before it is read)
            table_store.reset(); table_store_cap = 0;
            table_store.reset(static_cast<DevHuff*>(malloc((size_t)count * 6 * sizeof(DevHuff))));
            if (!table_store) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg: out of memory");
            table_store_cap = (size_t)count * 6;
        }
        for (int i = 0; i < count; ++i) b.prep[(size_t)i].huff = reinterpret_cast<DevHuff (*)[2]>(table_store.get() + (size_t)i * 6);
    }
    {
        ParserPool parsers(b.workers);
        parallel_for(count, b.workers, [&](int w, int i) { prepare_header(i, b.data[i], b.len[i], b.info[i], b.prep[(size_t)i], parsers[w]); });
    }
    for (int i = 0; i < count; ++i) if (b.prep[(size_t)i].progressive) { b.progressive.push_back(i); b.prep[(size_t)i].rc = kDeferred; }
    return GAMUT_HIP_OK;
}

// the hook owner places the coefficient buffers and chooses the hand-off per image (DecodeHooks::layout)
int plan_hand_off(BaselineBatch& b)
{
    const int count = b.count;
    b.tok.assign((size_t)count, 0); b.tok_off.assign((size_t)count, 0); b.strip_off.assign((size_t)count, 0); b.tok_cap.assign((size_t)count, 0);
    if (!(b.hooks && b.hooks->layout)) return GAMUT_HIP_OK;
    std::vector<int> rcs((size_t)count); std::vector<char> progs((size_t)count), tok_ok((size_t)count, 0);
    std::vector<size_t> scan_len((size_t)count, 0);
    for (int i = 0; i < count; ++i) {
        const FilePrep& fp = b.prep[(size_t)i];
        rcs[(size_t)i] = fp.rc == kDeferred || fp.rc == kHostRedo ? GAMUT_HIP_OK : fp.rc; progs[(size_t)i] = fp.progressive;
        tok_ok[(size_t)i] = fp.rc == GAMUT_HIP_OK && b.info[i].scan_type == GAMUT_JPGD_YH2V2 && fp.dev_unstuff && fp.items.size() == 1 && (uint32_t)fp.items[0].pad >= kSyncMinBytes;
        scan_len[(size_t)i] = fp.raw_len;
    }
    const TokenPlan plan{ tok_ok.data(), scan_len.data(), b.tok.data(), b.tok_off.data(), b.strip_off.data(), b.tok_cap.data(), &b.d_tokens, &b.d_strip_tab };
    return b.hooks->layout(b.info, rcs.data(), progs.data(), b.own_offsets.data(), b.own_offsets.data() + count, &b.d_coeffs, &b.d_max_zag, plan);
}

// B. serial: table de-duplication, slots of the files in the blob and in the raw image
void layout_tables_and_slots(BaselineBatch& b)
{
    const int count = b.count;
    b.images.resize((size_t)count);
    b.blob_off.assign((size_t)count, 0); b.raw_off.assign((size_t)count, 0);
    for (int i = 0; i < count; ++i) {
        const FilePrep& fp = b.prep[(size_t)i];
        DevImage& im = b.images[(size_t)i];
        memset(&im, 0, sizeof(im));
        if (fp.rc != GAMUT_HIP_OK) continue;
        b.any_ok = true;
        im.coeff_off = b.coeff_offset[i]; im.zag_off = b.zag_offset[i]; im.nb = fp.nb; im.org = (int32_t)fp.org;
        if (b.tok[(size_t)i]) {                                // strips = the reconstruction kernel's: 8 MCUs of 6 blocks along an MCU row
            im.tok = 1; im.tok_off = b.tok_off[(size_t)i]; im.strip_off = b.strip_off[(size_t)i]; im.tok_cap = b.tok_cap[(size_t)i];
            im.sb = 48; im.row_blocks = b.info[i].mcus_per_row * 6; im.n_strips = b.info[i].mcus_per_col * ((b.info[i].mcus_per_row + 7) / 8);
        }
        for (int c = 0; c < fp.comps; ++c) { im.quant[c] = intern(b.quants, fp.quant[c]); im.dc[c] = intern(b.huffs, fp.huff[c][0]); im.ac[c] = intern(b.huffs, fp.huff[c][1]); }
        b.blob_off[(size_t)i] = b.blob_size;
        b.blob_size += up16(fp.cap);
        b.max_items += fp.restart_interval ? (size_t)(fp.total_mcus / fp.restart_interval + 1) : 1;
        // files whose scan goes up as it is (k_jpeg_unstuff): their slots in the raw image, pinned and device
        if (fp.dev_unstuff) { b.raw_off[(size_t)i] = b.raw_size; b.raw_size += up16(fp.raw_len + 32); ++b.n_dev_files; }
    }
    b.ms_parse = ms_since(b.t_begin);
}

// the thread's staging for the call, and the status words the kernels flag errors in
int acquire_staging(BaselineBatch& b)
{
    const int count = b.count; const hipStream_t stream = b.stream;
    static thread_local PerDevice<hipStream_t> copy_stream_pd;
    hipStream_t& copy_stream = copy_stream_pd.cur();
    if (!copy_stream) GAMUT_HIP_CHECK(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    b.copy_stream = copy_stream;
    b.drain.arm(stream); b.drain.add(copy_stream);            // from here on every way out of the call waits for the streams it used
    static thread_local PerDevice<DeviceScratch> scratch_pd, raw_scratch_pd;
    static thread_local PerDevice<PinnedScratch> pinned_pd, raw_pinned_pd;
    b.d_blob = (uint8_t*)scratch_pd.cur().get(b.blob_size + kBlobSlack, stream);
    b.h_blob = pinned_pd.cur().get(b.blob_size + kBlobSlack, copy_stream);
    if (!b.d_blob || !b.h_blob) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg: staging allocation of %zu bytes failed", b.blob_size + kBlobSlack);
    if (b.n_dev_files) {
        b.d_raw = (uint8_t*)raw_scratch_pd.cur().get(b.raw_size + 64, stream);
        b.h_raw = raw_pinned_pd.cur().get(b.raw_size + 64, copy_stream);
        if (!b.d_raw || !b.h_raw) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg: staging allocation of %zu bytes failed", b.raw_size);
    }
    // (both kernels write every block of a segment as a whole line -- zeros included, blocks a damaged segment never reaches as
    // well: the coefficient buffer needs no clearing)
    uint32_t* st = b.d_status;
    if (!st) {                                                 // the kernels want somewhere to flag errors
        static thread_local PerDevice<DeviceScratch> sink_pd;
        st = (uint32_t*)sink_pd.cur().get((size_t)count * sizeof(uint32_t), stream);
        if (!st) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg: status allocation failed");
    }
    GAMUT_HIP_CHECK(hipMemsetAsync(st, 0, (size_t)count * sizeof(uint32_t), stream));
    static thread_local PerDevice<DeviceScratch> scan_end_pd;                     // per image: where k_jpeg_unstuff saw the scan end
    b.d_scan_end = (uint32_t*)scan_end_pd.cur().get((size_t)count * sizeof(uint32_t), stream);
    if (!b.d_scan_end) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg: status allocation failed");
    GAMUT_HIP_CHECK(hipMemsetAsync(b.d_scan_end, 0xFF, (size_t)count * sizeof(uint32_t), stream));
    b.st = st;
    return GAMUT_HIP_OK;
}

// C/D. groups of files.  A group's bytes are copied into pinned memory on the workers (as they are; files with tiny restart
//      intervals: unstuffed there) and DMA'd at once; its segment list follows and the group's kernels -- unstuff, entropy
//      decode, and through the hook the reconstruction -- are queued behind an event on a stream of the group's own, so the
//      first group decodes while the rest is still on its way.
int open_group_streams(BaselineBatch& b)
{
    const int count = b.count;
    static const int groups_env = env_int("GAMUT_HIP_JPEG_GROUPS", 0);        // measurements
    b.n_groups = groups_env > 0 ? std::min(kMaxGroups, std::min(groups_env, count)) : (count < 128 ? 1 : std::max(2, std::min(kMaxGroups, count / 256)));        // (1024 files, a stream per group: 4 groups 14.8 ms, 8 groups 16.1 ms, 2 groups 14.9 ms -- profiles/r04_jpeg_sweep.txt; three streams in turn: 4 groups 12.7 / 13.1, 6 groups 13.1 / 13.4, 8 groups 13.2 / 13.0; 256 files: 1 group 4.5, 2 groups 4.3, 4 groups 5.0 ms)
    struct EvN { hipEvent_t e[kMaxGroups]; }; struct StN { hipStream_t s[kMaxGroups]; };
    static thread_local PerDevice<EvN> group_ready_pd;
    b.group_ready = group_ready_pd.cur().e;
    for (int g = 0; g < b.n_groups; ++g) if (!b.group_ready[g]) GAMUT_HIP_CHECK(hipEventCreateWithFlags(&b.group_ready[g], hipEventDisableTiming));
    // A long segment is decoded by one workgroup in its own time (its sweeps), whatever else the chip does: the groups' kernels
    // are therefore queued on streams of their own (behind what `stream` holds now) and run side by side, each as soon as its
    // bytes are there -- on one stream a group waited for the group before it to finish.
    static thread_local PerDevice<StN> side_pd;
    static thread_local PerDevice<hipEvent_t> fork_pd;
    b.side = side_pd.cur().s;
    hipEvent_t& fork = fork_pd.cur();
    if (!fork) GAMUT_HIP_CHECK(hipEventCreateWithFlags(&fork, hipEventDisableTiming));
    // ... but not a stream per group: the runtime maps streams onto FOUR hardware queues (GPU_MAX_HW_QUEUES), a fifth stream shares one with
    // another, and its kernels wait for that stream's.  The timeline of round 4 (profiles/r04_jpeg_timeline.txt; rocprofv3 --kernel-trace
    // --memory-copy-trace): with `stream`, the copy stream and three side streams the LAST group's kernels started 4 ms after its bytes had
    // arrived, when the group before it had finished.  Three compute streams, taken in turn (a group's kernels take about as long as three
    // groups' uploads): 1024 files 14.0 / 13.6 -> 12.7 / 13.1 ms on one box (GAMUT_HIP_JPEG_STREAMS=5 is the old shape).  What is left is the
    // GPU's own time: side by side the groups' entropy kernels slow each other down (2.1 ms alone, 3.4 - 4.5 ms beside another one and a
    // reconstruction kernel) -- with four waves per SIMD the decode is bound by instruction issue, no longer by the length of a lane's chain.
    static const int lanes_env = env_int("GAMUT_HIP_JPEG_STREAMS", 0);        // measurements
    b.n_lanes = std::max(1, std::min(b.n_groups, lanes_env > 0 ? std::min(lanes_env, kMaxGroups) : 3));
    for (int g = 1; g < b.n_lanes; ++g) if (!b.side[g]) GAMUT_HIP_CHECK(hipStreamCreateWithFlags(&b.side[g], hipStreamNonBlocking));
    GAMUT_HIP_CHECK(hipEventRecord(fork, b.stream));
    for (int g = 1; g < b.n_lanes; ++g) { GAMUT_HIP_CHECK(hipStreamWaitEvent(b.side[g], fork, 0)); b.drain.add(b.side[g]); }
    return GAMUT_HIP_OK;
}

// one small pinned image of the tables: [images][huff][quant][raw-file records][items of group 0][items of group 1]...
int upload_tables(BaselineBatch& b)
{
    static thread_local PerDevice<DeviceScratch> tab_scratch_pd;
    static thread_local PerDevice<PinnedScratch> tab_pinned_pd;
    b.o_huff = up256(b.images.size() * sizeof(DevImage)); b.o_quant = up256(b.o_huff + b.huffs.size() * sizeof(DevHuff));
    b.o_raws = up256(b.o_quant + b.quants.size() * sizeof(QuantTab)); b.items_off = up256(b.o_raws + (size_t)b.n_dev_files * sizeof(DevRaw));
    b.tab_total = b.items_off + up256(b.max_items * sizeof(DevItem)) + 256 * (size_t)b.n_groups;
    b.d_tab = (uint8_t*)tab_scratch_pd.cur().get(b.tab_total, b.stream);
    b.h_tab = tab_pinned_pd.cur().get(b.tab_total, b.copy_stream);
    if (!b.d_tab || !b.h_tab) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg: staging allocation of %zu bytes failed", b.tab_total);
    memcpy(b.h_tab, b.images.data(), b.images.size() * sizeof(DevImage));
    memcpy(b.h_tab + b.o_huff, b.huffs.data(), b.huffs.size() * sizeof(DevHuff));
    memcpy(b.h_tab + b.o_quant, b.quants.data(), b.quants.size() * sizeof(QuantTab));
    GAMUT_HIP_CHECK(hipMemcpyAsync(b.d_tab, b.h_tab, b.o_raws, hipMemcpyHostToDevice, b.copy_stream));
    b.in_lds = b.n_huff() <= kLdsHuff && b.n_quant() <= kLdsQuant;
    return GAMUT_HIP_OK;
}

// files [g_lo, g_hi): their bytes into the pinned images, on the workers
void stage_group_bytes(BaselineBatch& b, int g_lo, int g_hi)
{
    parallel_for(g_hi - g_lo, b.workers, [&](int, int k) {
        const int i = g_lo + k;
        FilePrep& fp = b.prep[(size_t)i];
        if (fp.rc != GAMUT_HIP_OK) return;
        if (fp.dev_unstuff) memcpy(b.h_raw + b.raw_off[(size_t)i], b.data[i] + fp.scan_pos, fp.raw_len);
        else unstuff_file(i, b.data[i], b.len[i], fp, b.h_blob + b.blob_off[(size_t)i]);
    });
}

// the group's uploads: one DMA per run of neighbouring slots of the same kind
int upload_group(BaselineBatch& b, int g_lo, int g_hi)
{
    const std::vector<FilePrep>& prep = b.prep;
    int i = g_lo;
    while (i < g_hi) {
        const FilePrep& fp = prep[(size_t)i];
        if (fp.rc != GAMUT_HIP_OK || fp.used == 0) { ++i; continue; }
        const bool dev = fp.dev_unstuff;
        int j = i; size_t b0 = dev ? b.raw_off[(size_t)i] : b.blob_off[(size_t)i], b1 = b0;
        while (j < g_hi && (prep[(size_t)j].rc != GAMUT_HIP_OK || prep[(size_t)j].used == 0 || prep[(size_t)j].dev_unstuff == dev)) {
            const FilePrep& fj = prep[(size_t)j];
            if (fj.rc == GAMUT_HIP_OK && fj.used) b1 = dev ? b.raw_off[(size_t)j] + fj.raw_len : b.blob_off[(size_t)j] + fj.used;
            ++j;
        }
        if (b1 > b0) GAMUT_HIP_CHECK(hipMemcpyAsync((dev ? b.d_raw : b.d_blob) + b0, (dev ? b.h_raw : b.h_blob) + b0, b1 - b0, hipMemcpyHostToDevice, b.copy_stream));
        i = j;
    }
    return GAMUT_HIP_OK;
}

// the group's segment list: long segments get a workgroup each (self-synchronising decode), short ones a lane each
void build_group_items(BaselineBatch& b, int g_lo, int g_hi)
{
    std::vector<DevItem>& items = b.items;
    items.clear();
    for (int i = g_lo; i < g_hi; ++i) {
        const FilePrep& fp = b.prep[(size_t)i];
        if (fp.rc != GAMUT_HIP_OK) continue;
        for (DevItem it : fp.items) { if (!fp.dev_unstuff) { it.begin += b.blob_off[(size_t)i]; it.end += b.blob_off[(size_t)i]; } items.push_back(it); }
    }
    auto klass = [&](const DevItem& it) { return b.tok[(size_t)it.image] ? 0 : (uint32_t)it.pad >= kSyncMinBytes ? 1 : 2; };
    std::stable_sort(items.begin(), items.end(), [&](const DevItem& x, const DevItem& y) { return klass(x) < klass(y); });
    b.n_tok = 0;
    while (b.n_tok < (int)items.size() && klass(items[(size_t)b.n_tok]) == 0) ++b.n_tok;
    b.n_long = b.n_tok;
    while (b.n_long < (int)items.size() && klass(items[(size_t)b.n_long]) == 1) ++b.n_long;
    b.total_long += b.n_long; b.total_short += (int)items.size() - b.n_long;
}

// the files of the group that are unstuffed on the device: where their segments stand in the list (a file's segments
// are all of one class, the partition keeps their order)
void build_group_raws(BaselineBatch& b)
{
    const std::vector<DevItem>& items = b.items;
    const int n_items = (int)items.size();
    b.raws.clear();
    int k = 0;
    while (k < n_items) {
        const int img = items[(size_t)k].image; int e = k + 1;
        while (e < n_items && items[(size_t)e].image == img) ++e;
        const FilePrep& fp = b.prep[(size_t)img];
        if (fp.dev_unstuff) {
            DevRaw r; memset(&r, 0, sizeof(r));
            r.raw_begin = b.raw_off[(size_t)img]; r.raw_len = fp.raw_len; r.out_begin = b.blob_off[(size_t)img]; r.out_cap = up16(fp.cap);
            r.image = img; r.first_item = k; r.n_items = e - k; r.restart_interval = fp.restart_interval;
            b.raws.push_back(r);
        }
        k = e;
    }
}

// the group's two lists go up behind its bytes; its stream `gs` waits for all of them
int upload_group_lists(BaselineBatch& b, int g, hipStream_t gs)
{
    const size_t items_bytes = b.items.size() * sizeof(DevItem), raws_bytes = b.raws.size() * sizeof(DevRaw), raws_at = b.o_raws + (size_t)b.raws_done * sizeof(DevRaw);
    if (b.items_off + items_bytes > b.tab_total) return set_error(GAMUT_HIP_ERR_DECODE, "jpeg: more segments than the restart intervals allow");
    memcpy(b.h_tab + b.items_off, b.items.data(), items_bytes);
    GAMUT_HIP_CHECK(hipMemcpyAsync(b.d_tab + b.items_off, b.h_tab + b.items_off, items_bytes, hipMemcpyHostToDevice, b.copy_stream));
    b.d_items = (DevItem*)(b.d_tab + b.items_off);
    b.items_off = up256(b.items_off + items_bytes);
    b.d_raws = (const DevRaw*)(b.d_tab + raws_at);
    if (!b.raws.empty()) {
        if (b.raws_done + (int)b.raws.size() > b.n_dev_files) return set_error(GAMUT_HIP_ERR_DECODE, "jpeg: internal: raw-file records overflow");
        memcpy(b.h_tab + raws_at, b.raws.data(), raws_bytes);
        GAMUT_HIP_CHECK(hipMemcpyAsync(b.d_tab + raws_at, b.h_tab + raws_at, raws_bytes, hipMemcpyHostToDevice, b.copy_stream));
        b.raws_done += (int)b.raws.size();
    }
    GAMUT_HIP_CHECK(hipEventRecord(b.group_ready[g], b.copy_stream));
    GAMUT_HIP_CHECK(hipStreamWaitEvent(gs, b.group_ready[g], 0));
    return GAMUT_HIP_OK;
}

// `n` long segments from `d_items` on, a workgroup each; NH: how many tables the workgroup keeps in LDS (0: none)
template <bool TOK> int launch_entropy_sync(int nh_sel, const BaselineBatch& b, const DevItem* d_items, int n, int n_checkpoints, hipStream_t gs)
{
    uint32_t* const tokens = TOK ? b.d_tokens : nullptr; uint32_t* const strip_tab = TOK ? b.d_strip_tab : nullptr;
    const dim3 grid(n), block(kSyncThreads);
    if (nh_sel == 4)
        hipLaunchKernelGGL((k_jpeg_entropy_sync<4, TOK>), grid, block, 0, gs, d_items, b.d_img(), b.d_huff(), b.n_huff(), b.d_quant(), b.n_quant(), (const uint8_t*)b.d_blob, b.d_coeffs, b.d_max_zag, b.st, tokens, strip_tab, n_checkpoints);
    else if (nh_sel == kLdsHuff)
        hipLaunchKernelGGL((k_jpeg_entropy_sync<kLdsHuff, TOK>), grid, block, 0, gs, d_items, b.d_img(), b.d_huff(), b.n_huff(), b.d_quant(), b.n_quant(), (const uint8_t*)b.d_blob, b.d_coeffs, b.d_max_zag, b.st, tokens, strip_tab, n_checkpoints);
    else
        hipLaunchKernelGGL((k_jpeg_entropy_sync<0, TOK>), grid, block, 0, gs, d_items, b.d_img(), b.d_huff(), b.n_huff(), b.d_quant(), b.n_quant(), (const uint8_t*)b.d_blob, b.d_coeffs, b.d_max_zag, b.st, tokens, strip_tab, n_checkpoints);
    return launch_status(TOK ? "jpeg_entropy_sync (tokens)" : "jpeg_entropy_sync");
}

// the group's kernels on `gs`: unstuff, the three classes of segments, and through the hook the reconstruction
int launch_group(BaselineBatch& b, int g_lo, int g_hi, hipStream_t gs)
{
    const int n_items = (int)b.items.size(), n_tok = b.n_tok, n_long = b.n_long, n_short = n_items - n_long;
    if (b.trace) { (void)hipStreamSynchronize(gs); b.ms_upload = ms_since(b.t_up) - b.ms_kernels_issue; }
    const TracePoint t_k = trace_now();
    if (!b.raws.empty()) {
        hipLaunchKernelGGL(k_jpeg_unstuff, dim3((unsigned)b.raws.size()), dim3(kUnstuffThreads), 0, gs, b.d_raws, b.d_items, (const uint8_t*)b.d_raw, b.d_blob, b.st, b.d_scan_end);
        if (int rc = launch_status("jpeg_unstuff")) return rc;
    }
    static const int force_nh = env_int("GAMUT_HIP_JPEG_TABLES_LDS", -1);                  // measurements: 0 / 4 / 8
    const char* const ck_env = getenv("GAMUT_HIP_JPEG_CHECKPOINTS");                       // tests: checkpoints per lane of the counting passes (0 = the kernel's own)
    const int n_checkpoints = ck_env ? atoi(ck_env) : 0;
    const int nh_sel = force_nh == 0 ? 0 : (b.n_huff() <= 4 && b.n_quant() <= 4 && force_nh != 8) ? 4 : b.in_lds ? kLdsHuff : 0;
    if (n_tok)                                             // long segments of the images that hand over tokens
        if (int rc = launch_entropy_sync<true>(nh_sel, b, b.d_items, n_tok, n_checkpoints, gs)) return rc;
    if (n_long > n_tok)
        if (int rc = launch_entropy_sync<false>(nh_sel, b, b.d_items + n_tok, n_long - n_tok, n_checkpoints, gs)) return rc;
    if (n_short) {
        const dim3 grid((n_short + kEntropyThreads - 1) / kEntropyThreads), block(kEntropyThreads);
        if (b.in_lds) hipLaunchKernelGGL(k_jpeg_entropy<true>, grid, block, 0, gs, b.d_items + n_long, n_short, b.d_img(), b.d_huff(), b.n_huff(), b.d_quant(), b.n_quant(), (const uint8_t*)b.d_blob, b.d_coeffs, b.d_max_zag, b.st);
        else          hipLaunchKernelGGL(k_jpeg_entropy<false>, grid, block, 0, gs, b.d_items + n_long, n_short, b.d_img(), b.d_huff(), b.n_huff(), b.d_quant(), b.n_quant(), (const uint8_t*)b.d_blob, b.d_coeffs, b.d_max_zag, b.st);
    }
    if (int rc = launch_status("jpeg_entropy")) return rc;
    if (b.hooks && b.hooks->group_done) if (int rc = b.hooks->group_done(g_lo, g_hi, gs)) return rc;
    if (b.trace) { (void)hipStreamSynchronize(gs); b.ms_kernels_issue += ms_since(t_k); }
    return GAMUT_HIP_OK;
}

// What the kernels could not vouch for goes to the host feeder (redo_on_host): any flag (a bit pattern no code word begins, a run past coefficient 63, a
// segment that ran out, a wrong / missing RSTn, octets between an interval's last bit and its marker).  For the rest, find_eoi (:2826-2848):
// the markers behind the scan are processed like those in front of it -- nearly always FF D9 and nothing to do.
int collect_device_verdicts(BaselineBatch& b)
{
    const int count = b.count;
    std::vector<uint32_t> flags((size_t)count), ends((size_t)count);
    GAMUT_HIP_CHECK(hipMemcpy(flags.data(), b.st, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    GAMUT_HIP_CHECK(hipMemcpy(ends.data(), b.d_scan_end, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const bool redo_flagged = redo_flagged_files();
    for (int i = 0; i < count; ++i) {
        FilePrep& fp = b.prep[(size_t)i];
        if (fp.rc != GAMUT_HIP_OK) continue;
        if (flags[(size_t)i] && !redo_flagged) {
            fp.rc = GAMUT_HIP_ERR_DECODE; snprintf(fp.msg, sizeof(fp.msg), "image %d: jpeg: the entropy kernels flagged the scan (status %u), and the host feeder is switched off", i, flags[(size_t)i]);
            continue;
        }
        if (flags[(size_t)i]) { fp.rc = kHostRedo; continue; }
        const size_t n = b.len[i];
        const size_t e = fp.dev_unstuff ? (ends[(size_t)i] == 0xFFFFFFFFu ? n : fp.scan_pos + ends[(size_t)i]) : fp.scan_end;
        if (e >= n || (e + 1 < n && b.data[i][e] == 0xFF && b.data[i][e + 1] == 0xD9)) continue;        // the end of the file, or EOI at once
        std::unique_ptr<Parser> tp(new Parser());
        tp->data = b.data[i]; tp->len = n; tp->pos = e;
        if (next_scan(*tp, &b.info[i], Walk::kTrailer) < 0) { fp.rc = GAMUT_HIP_ERR_DECODE; snprintf(fp.msg, sizeof(fp.msg), "image %d: %s", i, last_error_buf()); }
    }
    return GAMUT_HIP_OK;
}

// the device pass over the files the kernels are given: staging, streams, tables, then group by group
int decode_on_device(BaselineBatch& b)
{
    b.t_up = trace_now();
    if (int rc = acquire_staging(b)) return rc;
    if (int rc = open_group_streams(b)) return rc;
    if (int rc = upload_tables(b)) return rc;
    for (int g = 0; g < b.n_groups; ++g) {
        const int g_lo = (int)((int64_t)b.count * g / b.n_groups), g_hi = (int)((int64_t)b.count * (g + 1) / b.n_groups);
        if (g_hi <= g_lo) continue;
        stage_group_bytes(b, g_lo, g_hi);
        if (int rc = upload_group(b, g_lo, g_hi)) return rc;
        build_group_items(b, g_lo, g_hi);
        if (b.items.empty()) continue;
        build_group_raws(b);
        const hipStream_t gs = g % b.n_lanes == 0 ? b.stream : b.side[g % b.n_lanes];
        if (int rc = upload_group_lists(b, g, gs)) return rc;
        if (int rc = launch_group(b, g_lo, g_hi, gs)) return rc;
    }
    GAMUT_HIP_CHECK(b.drain.wait());                       // copy stream, side streams, `stream`: the per-thread staging buffers are reused by the next call
    if (int rc = collect_device_verdicts(b)) return rc;
    if (b.trace) fprintf(stderr, "[gamut_hip] jpeg_entropy_decode_device: %d files in %d group(s), %d long + %d short segments, %d+%d tables, %.1f MB compressed, %d host threads: headers %.1f ms, unstuff + upload %.1f ms, kernels %.1f ms (stages serialised by the trace)\n",
                         b.count, b.n_groups, b.total_long, b.total_short, b.n_huff(), b.n_quant(), b.blob_size / 1e6, b.workers, b.ms_parse, b.ms_upload, b.ms_kernels_issue);
    return GAMUT_HIP_OK;
}

// the host feeder's files (see kHostRedo)
int redo_on_host(BaselineBatch& b)
{
    std::vector<int> redo;
    for (int i = 0; i < b.count; ++i) if (b.prep[(size_t)i].rc == kHostRedo) redo.push_back(i);
    if (redo.empty()) return GAMUT_HIP_OK;
    uint32_t* const stw = b.st ? b.st : b.d_status;
    const hipStream_t stream = b.stream; const DecodeHooks* const hooks = b.hooks;
    std::vector<int> rcs; std::vector<std::string> msgs;
    const auto deliver = hooks && hooks->redo ? std::function<int(int, const gamut_hip_jpeg_frame&)>([=](int i, const gamut_hip_jpeg_frame& fr) {
                             if (stw && hipMemsetAsync(stw + i, 0, sizeof(uint32_t), stream) != hipSuccess) return set_error(GAMUT_HIP_ERR_HIP, "jpeg: status reset failed");
                             return hooks->redo(i, fr, stream); })
                                              : deliver_dense(b.coeff_offset, b.zag_offset, b.d_coeffs, b.d_max_zag, stw, stream);
    if (int rc = host_redo(b.data, b.len, redo, b.info, deliver, rcs, msgs)) return rc;
    for (size_t k = 0; k < redo.size(); ++k) {
        FilePrep& fp = b.prep[(size_t)redo[k]];
        fp.rc = rcs[k];
        if (rcs[k] != GAMUT_HIP_OK) snprintf(fp.msg, sizeof(fp.msg), "image %d: %s", redo[k], msgs[k].c_str());
    }
    return GAMUT_HIP_OK;
}

// the verdicts of the baseline files into host_status; the lowest-numbered failure of the batch
struct FirstFailure { int rc = GAMUT_HIP_OK, index = -1; const char* msg = ""; };
FirstFailure fold_status(const BaselineBatch& b)
{
    FirstFailure first;
    for (int i = 0; i < b.count; ++i) {
        const FilePrep& fp = b.prep[(size_t)i];
        if (fp.rc == kDeferred) continue;
        if (b.host_status) b.host_status[i] = fp.rc;
        if (fp.rc != GAMUT_HIP_OK && first.rc == GAMUT_HIP_OK) { first.rc = fp.rc; first.msg = fp.msg; first.index = i; }
    }
    return first;
}

// the progressive files of the batch, into the same buffers; `first` moves to one of them if it fails in front of the baseline files' first
int hand_off_progressive(BaselineBatch& b, FirstFailure& first, char* prog_msg, size_t msg_cap)
{
    if (b.progressive.empty()) return GAMUT_HIP_OK;
    int prog_first = -1;
    const int rc = progressive_decode_device(b.data, b.len, b.progressive, b.coeff_offset, b.zag_offset, b.d_coeffs, b.d_max_zag, b.d_status, b.info, b.host_status, b.stream,
                                             &prog_first, prog_msg, msg_cap);
    if (rc != GAMUT_HIP_OK && prog_first < 0) return rc;                              // an allocation / HIP failure, message set
    if (rc != GAMUT_HIP_OK && (first.index < 0 || prog_first < first.index)) { first.rc = rc; first.msg = prog_msg; first.index = prog_first; }
    return GAMUT_HIP_OK;
}

int entropy_decode_device(const uint8_t* const* data, const size_t* len, int count,
                          const int64_t* coeff_offset_in, const int64_t* zag_offset_in,
                          int16_t* d_coeffs, uint8_t* d_max_zag, uint32_t* d_status,
                          gamut_hip_jpeg_frame* info, int* host_status, hipStream_t stream, const DecodeHooks* hooks = nullptr)
{
    BaselineBatch b{ data, len, count, coeff_offset_in, zag_offset_in, d_coeffs, d_max_zag, d_status, info, host_status, stream, hooks };
    if (hooks) { b.own_offsets.assign((size_t)count * 2, 0); b.coeff_offset = b.own_offsets.data(); b.zag_offset = b.own_offsets.data() + count; }
    if (!hooks && ((uintptr_t)d_coeffs & 15) != 0) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "jpeg_entropy_decode_device: the coefficient buffer must be 16-byte aligned");
    for (int i = 0; i < count && !hooks; ++i)
        if ((b.coeff_offset[i] & 7) != 0) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "jpeg_entropy_decode_device: coefficient offsets must be multiples of 8 elements (image %d)", i);

    if (int rc = prepare_headers(b)) return rc;
    if (int rc = plan_hand_off(b)) return rc;
    layout_tables_and_slots(b);
    // The caller's status words start out clear whatever happens below: a batch in which NO baseline file is the kernels' (every one
    // of them kHostRedo at prepare_header, or progressive) never reaches the clear of the device pass, and the file-level caller folds
    // these words into its verdicts -- stale memory there turned a file the host feeder had decoded into ERR_DECODE.
    if (d_status) GAMUT_HIP_CHECK(hipMemsetAsync(d_status, 0, (size_t)count * sizeof(uint32_t), stream));
    if (b.any_ok) if (int rc = decode_on_device(b)) return rc;
    if (int rc = redo_on_host(b)) return rc;
    FirstFailure first = fold_status(b);
    char prog_msg[256] = { 0 };
    if (int rc = hand_off_progressive(b, first, prog_msg, sizeof(prog_msg))) return rc;
    if (first.rc != GAMUT_HIP_OK) return set_error(first.rc, "%s", first.msg);
    return GAMUT_HIP_OK;
}

// A frame the host feeder decoded -> pixels in device memory at `out`: the coefficients and max_zag go up into scratch the thread
// keeps and through the dense reconstruction, all of it queued on `s`.  The sources are the frame's pageable buffers: the caller
// waits for `s` before it frees them.
int reconstruct_host_frame(const gamut_hip_jpeg_frame& fr, uint8_t* out, int out_comps, hipStream_t s)
{
    static thread_local PerDevice<DeviceScratch> co_pd, zz_pd;
    const size_t nblk = (size_t)fr.mcus_per_row * fr.mcus_per_col * fr.blocks_per_mcu;
    int16_t* c = (int16_t*)co_pd.cur().get(nblk * 128 + 256, s); uint8_t* z = (uint8_t*)zz_pd.cur().get(nblk + 256, s);
    if (!c || !z) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg: coefficient scratch of %zu blocks does not fit the device", nblk);
    GAMUT_HIP_CHECK(hipMemcpyAsync(c, fr.coeffs, nblk * 128, hipMemcpyHostToDevice, s));
    GAMUT_HIP_CHECK(hipMemcpyAsync(z, fr.max_zag, nblk, hipMemcpyHostToDevice, s));
    return jpeg_reconstruct_launch(c, (int64_t)nblk * 64, z, (int64_t)nblk, out, (int64_t)fr.width * out_comps, 0, fr.width, fr.height, fr.scan_type, out_comps, 1, s);
}
