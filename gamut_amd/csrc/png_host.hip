// png_host.hip -- device side of the PNG path as the host drives it, and its C-ABI entry points.
//
// The file itself -- the chunk walk of stbi__parse_png_file, the inflate of finalize_decode, which stay on the CPU in the reference
// too -- is png_file.hip's.  Everything after the inflate runs on
// the GPU: de-filter / expand (png.hip), Adam7 scatter, tRNS, palette, channel and depth
// conversion, in the order of finalize_decode (:1821-1857) and stbi__do_png (:2025-2055).
#include "png_file.hpp"
#include <map>
#include <mutex>
#include <tuple>

namespace gamut {
namespace {

struct Dev {
    void* p = nullptr;
    ~Dev() { if (p) (void)hipFree(p); }
    bool alloc(size_t n) { if (hipMalloc(&p, n ? n : 1) != hipSuccess) { p = nullptr; set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "png: hipMalloc(%zu) failed", n); return false; } return true; }
    void swap(Dev& o) { void* t = p; p = o.p; o.p = t; }
};

// The whole of stbi__do_png after the inflate, on the GPU: de-filter (+ Adam7), tRNS, palette, channel-count conversion
// (stbdec.d:1646-1679, 1821-1855, 2038-2045), then the 16 <-> 8 step of stbi__load_and_postprocess_* (:669-707) when
// want_bits (8 / 16; 0 = as decoded) asks for it.  The result is left at d_dst (device) or returned as malloc'd host memory.
uint8_t* png_run(const PngHeader& h, const uint8_t* raw, uint32_t raw_len, int req_comp, int want_bits, uint8_t* d_dst,
                 int* px, int* py, int* pn, int* bits_out, hipStream_t st, const uint8_t* d_raw = nullptr)
{
    const bool trace = trace_enabled();                                    // stage timings on stderr
    const auto now = trace_now;
    auto ms = [](TracePoint a, TracePoint b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    int img_n = h.img_n, out_n = png_out_channels(h, req_comp);
    int bytes = h.depth == 16 ? 2 : 1;
    const int64_t npx = (int64_t)h.x * h.y;

    const auto t1 = now();
    Dev draw, dimg, dstatus;
    if ((!d_raw && !draw.alloc((size_t)raw_len + 16)) || !dimg.alloc((size_t)npx * out_n * bytes + 16) || !dstatus.alloc(4)) return nullptr;
    const auto t2 = now();
    if ((!d_raw && hipMemcpyAsync(draw.p, raw, raw_len, hipMemcpyHostToDevice, st) != hipSuccess) || hipMemsetAsync(dstatus.p, 0, 4, st) != hipSuccess) {
        set_error(GAMUT_HIP_ERR_HIP, "png: upload failed"); return nullptr;
    }
    const uint8_t* const stream_dev = d_raw ? d_raw : (const uint8_t*)draw.p;      // the inflated stream in HBM
    if (trace) (void)hipStreamSynchronize(st);
    const auto t3 = now();
    if (!h.interlace) {
        if (png_defilter_launch(stream_dev, 0, raw_len, (uint8_t*)dimg.p, 0, h.x, h.y, img_n, out_n, h.depth, h.color, 1, (uint32_t*)dstatus.p, st)) return nullptr;
    } else {                                                              // stbi__create_png_image :1646-1679
        static const int xorig[7] = { 0,4,0,2,0,1,0 }, yorig[7] = { 0,0,4,0,2,0,1 }, xspc[7] = { 8,8,4,4,2,2,1 }, yspc[7] = { 8,8,8,4,4,2,2 };
        Dev dpass;
        if (!dpass.alloc((size_t)npx * out_n * bytes + 16)) return nullptr;
        const uint8_t* rp = stream_dev; uint32_t left = raw_len;
        for (int p = 0; p < 7; ++p) {
            const uint32_t x = (h.x - xorig[p] + xspc[p] - 1) / xspc[p], y = (h.y - yorig[p] + yspc[p] - 1) / yspc[p];
            if (!x || !y) continue;
            const uint32_t img_len = ((((uint32_t)img_n * x * h.depth) + 7) >> 3) * y + y;
            if (png_defilter_launch(rp, 0, left, (uint8_t*)dpass.p, 0, x, y, img_n, out_n, h.depth, h.color, 1, (uint32_t*)dstatus.p, st)) return nullptr;
            if (png_adam7_scatter_launch((const uint8_t*)dpass.p, (uint8_t*)dimg.p, x, y, h.x, out_n * bytes, p, st)) return nullptr;
            rp += img_len; left -= img_len;
        }
        if (hipStreamSynchronize(st) != hipSuccess) { set_error(GAMUT_HIP_ERR_HIP, "png: sync failed"); return nullptr; }   // dpass lifetime
    }
    if (h.has_trans && png_transparency_launch(dimg.p, npx, out_n, h.depth == 16, h.tc, st)) return nullptr;      // :1829-1841
    if (h.pal_img_n) {                                                      // :1843-1851
        img_n = h.pal_img_n; out_n = h.pal_img_n;
        if (req_comp >= 3) out_n = req_comp;
        Dev dpal, dexp;
        if (!dpal.alloc(1024) || !dexp.alloc((size_t)npx * out_n + 16)) return nullptr;
        if (hipMemcpyAsync(dpal.p, h.palette, 1024, hipMemcpyHostToDevice, st) != hipSuccess) { set_error(GAMUT_HIP_ERR_HIP, "png: upload failed"); return nullptr; }
        if (png_palette_launch((const uint8_t*)dimg.p, (uint8_t*)dexp.p, npx, out_n, (const uint8_t*)dpal.p, st)) return nullptr;
        if (hipStreamSynchronize(st) != hipSuccess) { set_error(GAMUT_HIP_ERR_HIP, "png: sync failed"); return nullptr; }   // dpal lifetime
        dimg.swap(dexp);
    } else if (h.has_trans) ++img_n;                                        // :1852-1855
    if (req_comp && req_comp != out_n) {                                    // stbi__do_png :2038-2045
        Dev dconv;
        if (!dconv.alloc((size_t)npx * req_comp * bytes + 16)) return nullptr;
        if (png_convert_format_launch(dimg.p, dconv.p, npx, out_n, req_comp, bytes == 2, st)) return nullptr;
        if (hipStreamSynchronize(st) != hipSuccess) { set_error(GAMUT_HIP_ERR_HIP, "png: sync failed"); return nullptr; }
        dimg.swap(dconv);
        out_n = req_comp;
    }
    int bits = h.depth <= 8 ? 8 : 16;
    if (want_bits && want_bits != bits) {                                   // stbi__convert_16_to_8 / _8_to_16 :635-666
        Dev ddepth;
        const int64_t samples = npx * out_n;
        if (!ddepth.alloc((size_t)samples * (want_bits / 8) + 16)) return nullptr;
        if (png_depth_convert_launch(dimg.p, ddepth.p, samples, want_bits == 16, st)) return nullptr;
        if (hipStreamSynchronize(st) != hipSuccess) { set_error(GAMUT_HIP_ERR_HIP, "png: sync failed"); return nullptr; }
        dimg.swap(ddepth);
        bits = want_bits; bytes = want_bits / 8;
    }
    if (trace) (void)hipStreamSynchronize(st);
    const auto t4 = now();
    const size_t out_bytes = (size_t)npx * out_n * bytes;
    uint8_t* result = d_dst ? d_dst : (uint8_t*)malloc(out_bytes ? out_bytes : 1);
    uint32_t status = 0;
    if (!result) { set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "png: out of memory"); return nullptr; }
    if (hipMemcpyAsync(result, dimg.p, out_bytes, d_dst ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(&status, dstatus.p, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) {
        if (!d_dst) free(result);
        set_error(GAMUT_HIP_ERR_HIP, "png: download failed: %s", hipGetErrorString(hipGetLastError())); return nullptr;
    }
    if (trace) fprintf(stderr, "[gamut_hip] png %ux%u: hipMalloc %.2f ms, upload %.2f, kernels %.2f, %s %.2f\n",
                       h.x, h.y, ms(t1, t2), ms(t2, t3), ms(t3, t4), d_dst ? "device copy" : "download", ms(t4, now()));
    if (status) { if (!d_dst) free(result); set_error(GAMUT_HIP_ERR_DECODE, "png: invalid filter"); return nullptr; }
    *px = (int)h.x; *py = (int)h.y; if (pn) *pn = img_n;
    *bits_out = bits;
    return result;
}

// stbi_load_from_memory / stbi_load_16_from_memory on one file: malloc'd host pixels of want_bits bits per sample
uint8_t* png_load(const uint8_t* data, size_t len, int* px, int* py, int* pn, int req_comp, int want_bits,
                  float* ppmX, float* ppmY, float* aspect)
{
    if (req_comp < 0 || req_comp > 4) { set_error(GAMUT_HIP_ERR_INVALID_ARG, "png: bad req_comp"); return nullptr; }
    PngHeader probe;
    if (parse(data, len, probe, true)) return nullptr;                       // a bad signature is reported as such with or without a GPU
    if (!have_device()) return nullptr;                                      // before any work: no GPU, no result
    struct Staging { HostBuf b{ nullptr, 0, true }; };
    static thread_local PerDevice<Staging> staging_pd;
    HostBuf& staging = staging_pd.cur().b;
    PngJob j; j.raw = staging;                                               // borrow the per-thread pinned buffer
    const TracePoint t0 = trace_now();
    const int rc = png_prepare(data, len, j);
    staging = j.raw; j.raw = HostBuf{};                                      // hand it back (it may have grown)
    if (rc != GAMUT_HIP_OK) return nullptr;
    if (trace_enabled()) fprintf(stderr, "[gamut_hip] png parse + inflate %.2f ms\n", ms_since(t0));
    if (ppmX) *ppmX = j.h.ppmX;
    if (ppmY) *ppmY = j.h.ppmY;
    if (aspect) *aspect = j.h.aspect;
    int bits = 8;
    return png_run(j.h, staging.p, j.raw_len, req_comp, want_bits, nullptr, px, py, pn, &bits, thread_stream());
}

// Pinned inflate buffers of the batch workers: taken for the duration of a call, kept for the next one (page-locking 30 MB
// costs milliseconds), never freed -- the HIP runtime may be gone at exit.
struct PinnedPool {
    std::mutex m; std::vector<HostBuf> idle;
    HostBuf take() { std::lock_guard<std::mutex> g(m); if (idle.empty()) return HostBuf{ nullptr, 0, true }; HostBuf b = idle.back(); idle.pop_back(); return b; }
    void give(const HostBuf& b) { std::lock_guard<std::mutex> g(m); idle.push_back(b); }
};
PinnedPool& pinned_pool() { static PinnedPool* p = new PinnedPool(); return *p; }

// Host threads that all run one callable, joined at the latest when the object goes out of scope: no way out of a stage leaves a thread
// behind that reads the stage's data.  A thread that cannot be started is done without -- the work is handed out dynamically, so
// the threads that did start (and the caller) take it.
struct HostThreads {
    std::vector<std::thread> pool;
    template <class Fn> int start(int n, Fn fn) { try { for (int t = 0; t < n; ++t) pool.emplace_back(fn); } catch (...) {} return (int)pool.size(); }
    void join() { for (std::thread& th : pool) th.join(); pool.clear(); }
    ~HostThreads() { join(); }
};
template <class Fn> void run_on_threads(int threads, Fn fn) { HostThreads pool; pool.start(threads - 1, fn); fn(); }      // the caller is one of them

// The events the compute stream waits on, one or two per slice round; destroyed on every way out.
struct SliceEvents {
    std::vector<hipEvent_t> ev;
    // a new event, recorded on `from`, that `to` waits for (false: HIP refused; what was made of the event is still owned)
    bool chain(hipStream_t from, hipStream_t to)
    {
        ev.push_back(nullptr);
        return hipEventCreateWithFlags(&ev.back(), hipEventDisableTiming) == hipSuccess && hipEventRecord(ev.back(), from) == hipSuccess &&
               hipStreamWaitEvent(to, ev.back(), 0) == hipSuccess;
    }
    void destroy() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); ev.clear(); }
    ~SliceEvents() { destroy(); }
};

// Batch: chunk walk + inflate on host threads, one file per thread at a time, into pinned memory; the inflated stream goes
// to a device arena at once (copy stream).  Files that need nothing but de-filter + expand (batched(), png_file.hpp) are then
// de-filtered TOGETHER, one launch per geometry with one workgroup per image (a 4K image alone occupies one CU for 4.5 ms; 64 of
// them side by side take about as long).  The others run the whole of stbi__do_png one after the other.
//
// Batches with more files than host threads inflate on the GPU (one workgroup per stream): a stream takes the kernel 0.8-3 times as long
// as it takes zlib on one host core, but up to 256 of them run side by side -- the host threads need a second round of files from
// threads + 1 files on (16 threads, 4K files: 16 files 64 / 40 ms on the host against 75 / 52 ms on the device, 24 files 112 / 67 against 75 / 51).
//
// One call of gamut_hip_png_decode_batch_device: what its stages share.  The stages, in the order of the entry point:
// plan_arena -> run_host_stage (inflate_worker | walk_worker) -> inflate_on_device (plan_device_inflate, launch_slices with
// upload_worker beside launch_round, collect_verdicts) -> defilter_batched -> decode_remaining -> report.
struct PngBatch {
    // the arguments
    const uint8_t* const* data; const size_t* len; int count, req_comp, bits;
    const int64_t* out_offset; uint8_t* out; gamut_hip_png_info* info; int* status_host; int threads; hipStream_t st;
    int dev = 0;
    // The calling thread's copy streams (per device).  Worker threads take them from here and never from a thread_local: a worker would
    // read ITS OWN (null) instance and upload on the legacy null stream.
    hipStream_t copy_stream = nullptr, copy_stream2 = nullptr;
    // per file: the verdict so far, the slot in the device arena for the inflated stream (-1: none)
    std::vector<BatchFile> files; std::vector<int64_t> slot, slot_bytes; int64_t arena_bytes = 0; uint8_t* d_arena = nullptr;
    // the host stage
    bool device_inflate = false; std::atomic<int> next{ 0 }; std::atomic<int64_t> us_inflate{ 0 }, us_upload{ 0 };
    // the device inflate: where the IDAT payloads lie in the files, the zlib stream of file i = its payloads without idat_skip[i] bytes
    std::vector<IdatSegments> segments; std::vector<uint32_t> idat_len, idat_skip;
    SlicePlan plan; uint8_t* h_blob = nullptr; uint8_t* d_blob = nullptr; uint32_t* d_verdict = nullptr;
    std::vector<std::atomic<int>> round_done; std::atomic<size_t> next_unit{ 0 }; std::atomic<bool> upload_failed{ false };
    std::vector<std::vector<uint32_t>> avail;              // (one table per launch, alive until the stream has been waited for)
    std::vector<uint32_t> verdict;                         // [0, n): inflated length, [n, 2n): status, per stream of the plan
    // the batched de-filter: files by geometry, their order in the launches, the offset tables and the status words
    std::map<std::tuple<uint32_t, uint32_t, int, int, int, int>, std::vector<int>> groups;
    std::vector<int> order; std::vector<int64_t> offs; std::vector<uint32_t> status; int n_batched = 0;
    // trace (GAMUT_HIP_TRACE)
    const bool trace = trace_enabled(); TracePoint t_begin; double ms_workers = 0, ms_device_inflate = 0;
    // Last, so that they go first: every way out of the call waits for the streams it used BEFORE the host memory above, which
    // downloads write into, is released; then the events go.
    SliceEvents events; StreamDrain drain;
};

// IHDR of every file: a slot in the device arena for its inflated stream
int plan_arena(PngBatch& b)
{
    static thread_local PerDevice<hipStream_t> copy_stream_pd;
    hipStream_t& copy_stream = copy_stream_pd.cur();
    if (!copy_stream) GAMUT_HIP_CHECK(hipStreamCreateWithFlags(&copy_stream, hipStreamNonBlocking));
    b.copy_stream = copy_stream;
    const size_t count = (size_t)b.count;
    b.files.resize(count); b.slot.assign(count, -1); b.slot_bytes.assign(count, 0);
    for (size_t i = 0; i < count; ++i) {
        PngHeader h;
        if (parse(b.data[i], b.len[i], h, true)) continue;                   // the worker reports the error
        const uint64_t room = h.slot_bytes();
        if (room > kMaxSlotBytes) continue;
        b.slot[i] = b.arena_bytes; b.slot_bytes[i] = (int64_t)room; b.arena_bytes += (int64_t)up256(room);
    }
    clear_error();
    static thread_local PerDevice<DeviceScratch> arena_pd;
    b.d_arena = b.arena_bytes ? (uint8_t*)arena_pd.cur().get((size_t)b.arena_bytes, b.st) : nullptr;
    if (b.arena_bytes && !b.d_arena) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "png: device arena of %lld bytes failed", (long long)b.arena_bytes);
    b.drain.arm(b.st); b.drain.add(b.copy_stream);          // from here on every way out of the call waits for the streams it used
    return GAMUT_HIP_OK;
}

// Host inflate: chunk walk + inflate into the worker's pinned buffer, and the stream goes to the arena at once
void inflate_worker(PngBatch& b)
{
    (void)hipSetDevice(b.dev);
    HostBuf buf = pinned_pool().take();
    hipEvent_t copied = nullptr;
    (void)hipEventCreateWithFlags(&copied, hipEventDisableTiming);
    for (int i; (i = b.next.fetch_add(1, std::memory_order_relaxed)) < b.count; ) {
        BatchFile& f = b.files[(size_t)i];
        PngJob j; j.raw = buf;                                           // borrow the worker's pinned buffer
        const TracePoint t_in = trace_now();
        const int rc = png_prepare(b.data[i], b.len[i], j);
        buf = j.raw; j.raw = HostBuf{};
        b.us_inflate += (int64_t)(ms_since(t_in) * 1000);
        if (rc != GAMUT_HIP_OK) { f.fail(i, rc, last_error_buf()); continue; }
        free(j.h.idata); j.h.idata = nullptr;
        f.accept(j.h, b.req_comp);
        if (b.slot[(size_t)i] < 0) { f.fail(i, GAMUT_HIP_ERR_DECODE, "png: image too large"); continue; }
        if (!copied) { f.fail(i, GAMUT_HIP_ERR_HIP, "png: event creation failed"); continue; }
        f.raw_len = (uint32_t)std::min<int64_t>((int64_t)j.raw_len, b.slot_bytes[(size_t)i]);
        const TracePoint t_upl = trace_now();
        if (hipMemcpyAsync(b.d_arena + b.slot[(size_t)i], buf.p, f.raw_len, hipMemcpyHostToDevice, b.copy_stream) != hipSuccess ||
            hipEventRecord(copied, b.copy_stream) != hipSuccess || hipEventSynchronize(copied) != hipSuccess) {
            f.fail(i, GAMUT_HIP_ERR_HIP, "png: upload failed"); continue;
        }
        b.us_upload += (int64_t)(ms_since(t_upl) * 1000);
        f.uploaded = true;
        f.batched = batched(f, b.req_comp, b.bits);
    }
    if (copied) (void)hipEventDestroy(copied);
    pinned_pool().give(buf);
}

// Device inflate, step one: the chunk walk of every file (no byte of IDAT data is touched: parse() notes where the payloads are)
void walk_worker(PngBatch& b)
{
    (void)hipSetDevice(b.dev);
    for (int i; (i = b.next.fetch_add(1, std::memory_order_relaxed)) < b.count; ) {
        BatchFile& f = b.files[(size_t)i];
        const IdatSegments& segments = b.segments[(size_t)i];
        PngHeader h;
        h.idat_segments = &b.segments[(size_t)i];
        const TracePoint t_in = trace_now();
        int rc = parse(b.data[i], b.len[i], h, false);
        if (rc == GAMUT_HIP_OK && !h.seen_idat) rc = set_error(GAMUT_HIP_ERR_DECODE, "png: no IDAT");
        uint32_t skip = 0;
        if (rc == GAMUT_HIP_OK && !h.is_iphone) {                       // the zlib header, as inflate_idat checks it
            uint8_t hd[2] = { 0, 0 };
            copy_idat_range(segments, 0, 0, std::min<uint32_t>(h.ioff, 2), hd);
            if (h.ioff < 2 || !zlib_header_ok(hd[0], hd[1])) rc = set_error(GAMUT_HIP_ERR_DECODE, "png: bad zlib header");
            skip = 2;
        }
        if (rc == GAMUT_HIP_OK && b.slot[(size_t)i] < 0) rc = set_error(GAMUT_HIP_ERR_DECODE, "png: image too large");
        if (rc != GAMUT_HIP_OK) { f.fail(i, rc, last_error_buf()); continue; }
        b.idat_len[(size_t)i] = h.ioff - skip;
        b.idat_skip[(size_t)i] = skip;
        h.idat_segments = nullptr;
        f.accept(h, b.req_comp);
        b.us_inflate += (int64_t)(ms_since(t_in) * 1000);
    }
}

// The host stage: the files over the host threads.  Inflate on the GPU (inflate.hip) when the batch is large enough to beat the host
// threads: the workers then only walk the chunks.  GAMUT_HIP_PNG_INFLATE=host / device overrides the choice.
int run_host_stage(PngBatch& b)
{
    b.t_begin = trace_now();
    b.device_inflate = b.count > b.threads;                  // (threads <= count here)
    if (const char* v = getenv("GAMUT_HIP_PNG_INFLATE")) b.device_inflate = strcmp(v, "device") == 0 ? true : strcmp(v, "host") == 0 ? false : b.device_inflate;
    b.idat_len.assign((size_t)b.count, 0); b.idat_skip.assign((size_t)b.count, 0);
    if (b.device_inflate) {
        b.segments.resize((size_t)b.count);
        run_on_threads(b.threads, [&b] { walk_worker(b); });
    } else {
        run_on_threads(b.threads, [&b] { inflate_worker(b); });
    }
    clear_error();
    GAMUT_HIP_CHECK(hipStreamSynchronize(b.copy_stream));                         // (every worker waited for its own copies already)
    return GAMUT_HIP_OK;
}

// Device inflate, the plan: which streams, the slices and the layout of the staging image (plan_slices), the staging itself
int plan_device_inflate(PngBatch& b)
{
    std::vector<int> streams;
    for (int i = 0; i < b.count; ++i) if (b.files[(size_t)i].rc == GAMUT_HIP_OK) streams.push_back(i);
    if (streams.empty()) return GAMUT_HIP_OK;
    static thread_local PerDevice<DeviceScratch> verdict_dev_pd;
    b.d_verdict = (uint32_t*)verdict_dev_pd.cur().get(streams.size() * 8);
    if (!b.d_verdict) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "png: verdict table allocation failed");
    SliceOverrides ov;
    if (const char* v = getenv("GAMUT_HIP_PNG_SLICE_KB")) { const long kb = atol(v); if (kb >= 64 && kb <= (1 << 20)) ov.slice = (uint32_t)kb << 10; }      // (tuning)
    if (const char* v = getenv("GAMUT_HIP_PNG_PITCHED")) ov.pitched = atoi(v) != 0;                            // (measurements)
    b.plan = plan_slices(b.idat_len, b.slot_bytes, streams, ov);
    static thread_local PerDevice<PinnedScratch> blob_pinned_pd;
    static thread_local PerDevice<DeviceScratch> blob_dev_pd;
    b.h_blob = blob_pinned_pd.cur().get(b.plan.blob_bytes + 16);
    b.d_blob = (uint8_t*)blob_dev_pd.cur().get(b.plan.blob_bytes + 16);
    if (!b.h_blob || !b.d_blob) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "png: staging for %llu bytes of IDAT data failed", (unsigned long long)b.plan.blob_bytes);
    static thread_local PerDevice<hipStream_t> copy2_pd;
    hipStream_t& copy_stream2 = copy2_pd.cur();
    if (!copy_stream2 && hipStreamCreateWithFlags(&copy_stream2, hipStreamNonBlocking) != hipSuccess) return set_error(GAMUT_HIP_ERR_HIP, "png: stream creation failed");
    b.copy_stream2 = copy_stream2;
    b.drain.add(b.copy_stream2);
    b.round_done = std::vector<std::atomic<int>>((size_t)b.plan.rounds);
    for (auto& a : b.round_done) a.store(0);
    return GAMUT_HIP_OK;
}

// The upload threads: a unit is slice r of one stream, gathered from the file's IDAT chunks into the pinned image; tight layout: and
// queued for upload at once, on the two copy streams in turn
void upload_worker(PngBatch& b)
{
    (void)hipSetDevice(b.dev);
    const SlicePlan& p = b.plan;
    for (size_t u; (u = b.next_unit.fetch_add(1, std::memory_order_relaxed)) < p.units.size(); ) {
        const int r = p.units[u].first, k = p.units[u].second, i = p.who[(size_t)k];
        const uint64_t lo = (uint64_t)r * p.slice, hi = p.avail(r, (size_t)k);        // the unit's bytes of the stream
        uint8_t* const dst = b.h_blob + p.blob_off[(size_t)i] + lo;
        copy_idat_range(b.segments[(size_t)i], b.idat_skip[(size_t)i], lo, hi, dst);
        if (!p.pitched && hi > lo && hipMemcpyAsync(b.d_blob + p.blob_off[(size_t)i] + lo, dst, (size_t)(hi - lo), hipMemcpyHostToDevice, (u & 1) ? b.copy_stream2 : b.copy_stream) != hipSuccess) {
            (void)hipGetLastError(); b.upload_failed.store(true);
        }
        b.round_done[(size_t)r].fetch_add(1, std::memory_order_release);
    }
}

// Round r of the launch loop.  Once slice r of every stream is in the pinned image (pitched: it goes up now, in one copy) / has been
// queued on the copy streams, the compute stream waits for it, then inflates what is there.
int launch_round(PngBatch& b, int r)
{
    const SlicePlan& p = b.plan;
    const size_t n = p.who.size(); const int active = p.units_in_round[(size_t)r];
    while (b.round_done[(size_t)r].load(std::memory_order_acquire) < active) std::this_thread::yield();
    if (p.pitched && active > 0 &&
        hipMemcpy2DAsync(b.d_blob + (uint64_t)r * p.slice, p.pitch, b.h_blob + (uint64_t)r * p.slice, p.pitch, p.slice, (size_t)active, hipMemcpyHostToDevice, b.copy_stream) != hipSuccess) {
        (void)hipGetLastError(); return set_error(GAMUT_HIP_ERR_HIP, "png: upload of slice %d failed", r);
    }
    if (!b.events.chain(b.copy_stream, b.st) || (!p.pitched && !b.events.chain(b.copy_stream2, b.st))) {
        (void)hipGetLastError(); return set_error(GAMUT_HIP_ERR_HIP, "png: event for slice %d failed", r);
    }
    std::vector<uint32_t>& avail = b.avail[(size_t)r];
    avail.resize(n);
    for (size_t k = 0; k < n; ++k) avail[k] = p.avail(r, k);
    return inflate_sliced_step((int)n, avail.data(), b.d_verdict, b.d_verdict + n, b.st);
}

// Device inflate, step two: the IDAT bytes go up slice by slice on the upload threads and the inflate kernel is launched once per slice
// behind them (inflate_sliced_*: a stream stops where the bytes it may read end and goes on in the next launch).  A stream inflates at
// ~150-600 MB/s, all of them side by side: about what PCIe delivers to all of them together, so the upload hides behind the kernel
// instead of standing in front of it.  Returns once every stream of the call has been waited for.
int launch_slices(PngBatch& b)
{
    const SlicePlan& p = b.plan;
    const size_t n = p.who.size();
    std::vector<gamut_hip_inflate_desc> descs;
    for (int i : p.who) descs.push_back(gamut_hip_inflate_desc{ b.d_blob + p.blob_off[(size_t)i], b.d_arena + b.slot[(size_t)i], b.idat_len[(size_t)i], (uint32_t)b.slot_bytes[(size_t)i] });
    b.verdict.resize(n * 2); b.avail.resize((size_t)p.rounds);
    if (int rc = inflate_sliced_begin(descs.data(), (int)n, b.st)) return rc;
    HostThreads pool;
    if (pool.start(b.threads, [&b] { upload_worker(b); }) == 0) upload_worker(b);      // (no thread could be started: this one does it all, then launches)
    int launch_rc = GAMUT_HIP_OK;
    for (int r = 0; r < p.rounds && launch_rc == GAMUT_HIP_OK; ++r) launch_rc = launch_round(b, r);
    pool.join();
    if (launch_rc == GAMUT_HIP_OK && b.upload_failed.load()) launch_rc = set_error(GAMUT_HIP_ERR_HIP, "png: upload of the IDAT data failed");
    if (launch_rc == GAMUT_HIP_OK && hipMemcpyAsync(b.verdict.data(), b.d_verdict, n * 8, hipMemcpyDeviceToHost, b.st) != hipSuccess) launch_rc = set_error(GAMUT_HIP_ERR_HIP, "png: verdict download failed");
    const hipError_t sync_rc = hipStreamSynchronize(b.st);
    (void)hipStreamSynchronize(b.copy_stream); (void)hipStreamSynchronize(b.copy_stream2);
    b.events.destroy();
    if (launch_rc != GAMUT_HIP_OK) return launch_rc;
    if (sync_rc != hipSuccess) return set_error(GAMUT_HIP_ERR_HIP, "png: inflate on the device failed: %s", hipGetErrorString(sync_rc));
    return GAMUT_HIP_OK;
}

// what the inflate kernel made of every stream: its length in the arena, or a damaged stream
void collect_verdicts(PngBatch& b)
{
    const size_t n = b.plan.who.size();
    for (size_t k = 0; k < n; ++k) {
        const int i = b.plan.who[k];
        BatchFile& f = b.files[(size_t)i];
        if (b.verdict[n + k]) { f.fail(i, GAMUT_HIP_ERR_DECODE, "png: corrupt zlib stream"); continue; }
        f.raw_len = b.verdict[k];
        f.uploaded = true;
        f.batched = batched(f, b.req_comp, b.bits);
    }
}

int inflate_on_device(PngBatch& b)
{
    const TracePoint t_inf = trace_now();
    if (int rc = plan_device_inflate(b)) return rc;
    if (!b.plan.who.empty()) {
        if (int rc = launch_slices(b)) return rc;
        collect_verdicts(b);
    }
    b.ms_device_inflate = ms_since(t_inf);
    return GAMUT_HIP_OK;
}

// the batched files by geometry, in the order of their launches: where each one's stream lies in the arena and where its pixels go.
// aligned / lines: every image on a dword / on a 128-byte line of memory
void group_by_geometry(PngBatch& b, bool& aligned, bool& lines)
{
    aligned = ((uintptr_t)b.out % 4) == 0; lines = ((uintptr_t)b.out % 128) == 0;
    for (int i = 0; i < b.count; ++i) {
        const BatchFile& f = b.files[(size_t)i];
        if (!f.batched) continue;
        b.groups[std::make_tuple(f.h.x, f.h.y, f.h.img_n, f.out_n, f.h.depth, f.h.color)].push_back(i);
        aligned = aligned && (b.out_offset[i] % 4) == 0;
        lines = lines && (b.out_offset[i] % 128) == 0;
        ++b.n_batched;
    }
    const size_t nb = (size_t)b.n_batched;
    b.status.assign(nb, 0); b.offs.resize(nb * 2); b.order.reserve(nb);
    for (auto& g : b.groups) for (int i : g.second) { b.offs[b.order.size()] = b.slot[(size_t)i]; b.offs[nb + b.order.size()] = b.out_offset[i]; b.order.push_back(i); }
}

// one de-filter launch per geometry
int defilter_batched(PngBatch& b)
{
    bool aligned, lines;
    group_by_geometry(b, aligned, lines);
    if (!b.n_batched) return GAMUT_HIP_OK;
    const size_t nb = (size_t)b.n_batched, o_status = nb * 16;
    static thread_local PerDevice<DeviceScratch> tables_pd;
    uint8_t* d_tab = (uint8_t*)tables_pd.cur().get(o_status + nb * 4);
    if (!d_tab) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "png: table allocation failed");
    GAMUT_HIP_CHECK(hipMemcpyAsync(d_tab, b.offs.data(), b.offs.size() * 8, hipMemcpyHostToDevice, b.st));
    GAMUT_HIP_CHECK(hipMemsetAsync(d_tab + o_status, 0, nb * 4, b.st));
    size_t base = 0; int launch_rc = GAMUT_HIP_OK;
    for (auto& g : b.groups) {
        const BatchFile& f = b.files[(size_t)g.second[0]];
        const int n = (int)g.second.size();
        const int rc = png_defilter_launch(b.d_arena, 0, f.need, b.out, 0, f.h.x, f.h.y, f.h.img_n, f.out_n, f.h.depth, f.h.color, n,
                                           (uint32_t*)(d_tab + o_status) + base, b.st,
                                           (const int64_t*)d_tab + base, (const int64_t*)d_tab + nb + base, aligned, lines);
        if (rc != GAMUT_HIP_OK && launch_rc == GAMUT_HIP_OK) {
            launch_rc = rc;
            for (int i : g.second) b.files[(size_t)i].fail(i, rc, last_error_buf());
        }
        base += (size_t)n;
    }
    GAMUT_HIP_CHECK(hipMemcpyAsync(b.status.data(), d_tab + o_status, nb * 4, hipMemcpyDeviceToHost, b.st));
    GAMUT_HIP_CHECK(hipStreamSynchronize(b.st));
    for (size_t k = 0; k < b.order.size(); ++k) {
        BatchFile& f = b.files[(size_t)b.order[k]];
        if (b.status[k] && f.rc == GAMUT_HIP_OK) f.fail(b.order[k], GAMUT_HIP_ERR_DECODE, "png: invalid filter");
    }
    return GAMUT_HIP_OK;
}

// the others (interlaced, palette, tRNS, channel or depth conversion): the whole of stbi__do_png per file, from the arena
void decode_remaining(PngBatch& b)
{
    for (int i = 0; i < b.count; ++i) {
        BatchFile& f = b.files[(size_t)i];
        if (f.rc != GAMUT_HIP_OK || !f.uploaded || f.batched) continue;
        int w = 0, hh = 0, n = 0, bits = 8;
        if (png_run(f.h, nullptr, f.raw_len, b.req_comp, b.bits, b.out + b.out_offset[i], &w, &hh, &n, &bits, b.st, b.d_arena + b.slot[(size_t)i])) { f.channels_in_file = n; f.bits = bits; }
        else f.fail(i, GAMUT_HIP_ERR_DECODE, last_error_buf());
    }
    clear_error();
}

// the results: info and status per file; the call's verdict is the first failing file's
int report(PngBatch& b)
{
    if (b.trace && b.device_inflate) fprintf(stderr, "[gamut_hip] png_decode_batch_device: inflate on the device: upload + kernel + verdicts %.1f ms\n", b.ms_device_inflate);
    if (b.trace) fprintf(stderr, "[gamut_hip] png_decode_batch_device: %d files on %d threads: workers %.1f ms (per file: chunk walk + inflate %.1f ms, upload + wait %.1f ms), GPU stages %.1f ms (%d files in %d batched launches)\n",
                         b.count, b.threads, b.ms_workers, b.us_inflate.load() / 1000.0 / b.count, b.us_upload.load() / 1000.0 / b.count, ms_since(b.t_begin) - b.ms_workers, b.n_batched, (int)b.groups.size());
    const BatchFile* first = nullptr;
    for (int i = 0; i < b.count; ++i) {
        const BatchFile& f = b.files[(size_t)i];
        gamut_hip_png_info& info = b.info[i];
        memset(&info, 0, sizeof(info));
        if (f.rc == GAMUT_HIP_OK) {
            info.width = f.h.x; info.height = f.h.y; info.channels_in_file = f.channels_in_file;
            info.channels = b.req_comp ? b.req_comp : f.channels_in_file; info.bits = f.bits;
            info.pixels_per_meter_x = f.h.ppmX; info.pixels_per_meter_y = f.h.ppmY; info.pixel_aspect_ratio = f.h.aspect;
        }
        if (b.status_host) b.status_host[i] = f.rc;
        if (f.rc != GAMUT_HIP_OK && !first) first = &f;
    }
    return first ? set_error(first->rc, "%s", first->msg) : GAMUT_HIP_OK;
}

} // namespace
} // namespace gamut

using namespace gamut;

extern "C" {

int gamut_hip_png_defilter_batch_device(const uint8_t* raw, int64_t raw_stride, uint32_t raw_len,
                                        uint8_t* out, int64_t out_stride,
                                        uint32_t x, uint32_t y, int img_n, int out_n, int depth, int color,
                                        int count, uint32_t* status, void* stream)
{
    clear_error();
    return png_defilter_launch(raw, raw_stride, raw_len, out, out_stride, x, y, img_n, out_n, depth, color, count, status, pick_stream(stream));
}

int gamut_hip_png_defilter_device(const gamut_hip_png_desc* descs, int count, uint32_t* status, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && !descs)) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "png_defilter: bad descriptor array");
    for (int i = 0; i < count; ++i) {
        const gamut_hip_png_desc& d = descs[i];
        if (int rc = png_defilter_launch(d.raw, 0, d.raw_len, d.out, 0, d.x, d.y, d.img_n, d.out_n, d.depth, d.color, 1,
                                         status ? status + i : nullptr, pick_stream(stream)))
            return rc;
    }
    return GAMUT_HIP_OK;
}

uint8_t* gamut_hip_stbi_load_from_memory(const uint8_t* data, size_t len, int* x, int* y, int* comp, int req_comp,
                                         float* ppmX, float* ppmY, float* pixelRatio)
{
    clear_error();
    int n = 0, w = 0, h = 0;
    uint8_t* r = png_load(data, len, &w, &h, &n, req_comp, 8, ppmX, ppmY, pixelRatio);         // 16-bit files: stbi__convert_16_to_8
    if (!r) return nullptr;
    if (x) *x = w;
    if (y) *y = h;
    if (comp) *comp = n;
    return r;
}

uint16_t* gamut_hip_stbi_load_16_from_memory(const uint8_t* data, size_t len, int* x, int* y, int* comp, int req_comp,
                                             float* ppmX, float* ppmY, float* pixelRatio)
{
    clear_error();
    int n = 0, w = 0, h = 0;
    uint8_t* r = png_load(data, len, &w, &h, &n, req_comp, 16, ppmX, ppmY, pixelRatio);        // 8-bit files: stbi__convert_8_to_16
    if (!r) return nullptr;
    if (x) *x = w;
    if (y) *y = h;
    if (comp) *comp = n;
    return (uint16_t*)r;
}

// files -> pixels in device memory (PngBatch above: the stages and what they share)
int gamut_hip_png_decode_batch_device(const uint8_t* const* data, const size_t* len, int count, int req_comp, int bits,
                                      const int64_t* out_offset, uint8_t* out, gamut_hip_png_info* info, int* status_host,
                                      int threads, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!data || !len || !out_offset || !out || !info)) || req_comp < 0 || req_comp > 4 || (bits != 0 && bits != 8 && bits != 16))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "png_decode_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        if (threads <= 0) threads = host_threads();
        threads = threads < 1 ? 1 : threads > count ? count : threads;
        PngBatch b{ data, len, count, req_comp, bits, out_offset, out, info, status_host, threads, pick_stream(stream) };
        (void)hipGetDevice(&b.dev);
        if (int rc = plan_arena(b)) return rc;
        if (int rc = run_host_stage(b)) return rc;
        if (b.device_inflate) if (int rc = inflate_on_device(b)) return rc;
        b.ms_workers = ms_since(b.t_begin);
        if (int rc = defilter_batched(b)) return rc;
        decode_remaining(b);
        return report(b);
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "png_decode_batch_device: out of host memory");
    }
}

int gamut_hip_png_read_header(const uint8_t* data, size_t len, gamut_hip_png_info* info)
{
    clear_error();
    if (!info) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "png_read_header: null info");
    memset(info, 0, sizeof(*info));
    PngHeader h;
    if (int rc = parse(data, len, h, true)) return rc;
    info->width = h.x; info->height = h.y; info->bits = h.depth == 16 ? 16 : 8;
    info->channels_in_file = info->channels = h.color == 3 ? 3 : h.img_n;          // palette images expand to RGB (RGBA with tRNS: known after the chunk walk)
    info->pixels_per_meter_x = info->pixels_per_meter_y = info->pixel_aspect_ratio = -1;
    return GAMUT_HIP_OK;
}

int gamut_hip_png_is16(const uint8_t* data, size_t len)
{
    PngHeader h;
    if (parse(data, len, h, true)) { clear_error(); return 0; }
    return h.depth == 16 ? 1 : 0;
}

} // extern "C"