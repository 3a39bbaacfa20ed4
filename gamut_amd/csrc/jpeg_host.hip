// jpeg_host.hip -- host side of the JPEG path: the baseline entropy-decode feeder that
// produces the dense coefficient form the kernels consume, and the C-ABI entry points.
//
// The feeder does what jpeg_decoder::decode_next_row does on the CPU in the reference
// (jpegload.d:2405-2525: Huffman decode, DC prediction, de-quantise `s * q[k]` into natural
// order through g_ZAG, track m_mcu_block_max_zag), for a whole image at once, after the
// marker pass of :1160-1848 (DQT tables kept in zig-zag order as int16, :1313-1329; DHT;
// SOF0/SOF1 8-bit; DRI; SOS).  It stays on the host: bit-serial work.
// Progressive frames (SOF2, jpegload.d:3296-3664) accumulate their scans into per-component coefficient planes on the
// host and come out in the same dense form, so the kernels do not know the difference.
// Not supported (the call fails like the reference fails on a stream it rejects): arithmetic / lossless /
// hierarchical frames, 12-bit precision, CMYK, multi-scan *baseline* files.
//
// One translation unit in four layers, each a header included below inside the same anonymous namespace: jpeg_parse.hpp (the host
// parser and feeder), jpeg_entropy_kernels.hpp (device structs and kernels of the baseline decode), jpeg_batch.hpp (the batch
// orchestration, entropy_decode_device), jpeg_prog.hpp (the progressive decode on the device).  This file keeps the C entry points.
#include "common.hpp"
#include <functional>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <memory>
#include <new>
#include <string>
#include <thread>
#include <vector>

namespace gamut {
namespace {

#include "jpeg_parse.hpp"
#include "jpeg_entropy_kernels.hpp"
#include "jpeg_batch.hpp"
#include "jpeg_prog.hpp"

} // namespace
} // namespace gamut

using namespace gamut;

#if JPEG_SYNC_PROFILE
extern "C" int gamut_hip_jpeg_sync_profile(unsigned long long* out8, int reset)      // measurement builds only
{
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(g_sync_prof), 128) != hipSuccess) return 1;          // (sixteen counters)
    if (reset) { unsigned long long z[16] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(g_sync_prof), z, 128) != hipSuccess) return 1; }
    return 0;
}
#endif
extern "C" {

int gamut_hip_jpeg_decode_coeffs(const uint8_t* data, size_t len, gamut_hip_jpeg_frame* out)
{
    clear_error();
    if (!out) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "jpeg_decode_coeffs: null frame");
    return decode_coeffs(data, len, out);
}

int gamut_hip_jpeg_decode_coeffs_batch(const uint8_t* const* data, const size_t* len, int count,
                                       gamut_hip_jpeg_frame* out, int* status, int threads)
{
    clear_error();
    if (count < 0 || (count > 0 && (!data || !len || !out)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "jpeg_decode_coeffs_batch: bad arguments");
    if (threads <= 0) threads = host_threads();
    if (threads < 1) threads = 1;
    if (threads > count) threads = count;
    try {
    // images are independent: workers pull the next index; every worker keeps the message of its lowest failing image
    std::atomic<int> next{ 0 };
    struct Failure { int index = INT32_MAX, code = GAMUT_HIP_OK; char msg[256] = { 0 }; };
    std::vector<Failure> fails((size_t)(threads > 0 ? threads : 1));
    auto work = [&](int tid) {
        for (int i; (i = next.fetch_add(1, std::memory_order_relaxed)) < count; ) {
            const int rc = decode_coeffs(data[i], len[i], &out[i]);
            if (status) status[i] = rc;
            if (rc != GAMUT_HIP_OK && i < fails[tid].index) {
                fails[tid].index = i; fails[tid].code = rc;
                snprintf(fails[tid].msg, sizeof(fails[tid].msg), "%s", last_error_buf());       // this worker thread's message
            }
        }
    };
    if (threads <= 1) { if (count > 0) work(0); }
    else {
        std::vector<std::thread> pool;
        pool.reserve((size_t)threads - 1);
        try {                                                  // thread creation may fail (EAGAIN): the rest runs on fewer workers
            for (int t = 1; t < threads; ++t) pool.emplace_back(work, t);
        } catch (...) {}
        work(0);
        for (std::thread& th : pool) th.join();
    }
    const Failure* first = nullptr;
    for (const Failure& fl : fails) if (fl.code != GAMUT_HIP_OK && (!first || fl.index < first->index)) first = &fl;
    if (!first) { clear_error(); return GAMUT_HIP_OK; }
    return set_error(first->code, "image %d: %s", first->index, first->msg);
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg_decode_coeffs_batch: out of host memory");
    }
}

int gamut_hip_jpeg_read_header(const uint8_t* data, size_t len, gamut_hip_jpeg_frame* out)
{
    clear_error();
    if (!out) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "jpeg_read_header: null frame");
    Parser* ps = new (std::nothrow) Parser();
    if (!ps) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg: out of memory");
    const int rc = parse_baseline(*ps, data, len, out, false);
    delete ps;
    return rc;
}

int gamut_hip_jpeg_scan_layout(const uint8_t* data, size_t len, gamut_hip_jpeg_frame* info, int32_t* segments, uint64_t* entropy_bytes)
{
    clear_error();
    if (!info) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "jpeg_scan_layout: null frame");
    try {
        Parser* ps = new Parser();
        FilePrep fp;
        std::vector<DevHuff> fp_tables(6);
        fp.huff = reinterpret_cast<DevHuff (*)[2]>(fp_tables.data());
        prepare_header(0, data, len, *info, fp, *ps);
        delete ps;
        if (fp.progressive) {                                  // every scan of the file, cut at its restart markers (jpeg_prog.hpp)
            Parser* pp = new Parser();
            ProgPrep pr;
            prog_prepare(0, data, len, *info, pr, *pp);
            delete pp;
            std::vector<uint8_t> bytes(pr.rc == GAMUT_HIP_OK ? pr.cap : 0);
            if (pr.rc == GAMUT_HIP_OK) prog_unstuff(0, data, pr, bytes.data());
            if (segments) *segments = (int32_t)pr.items.size();
            if (entropy_bytes) *entropy_bytes = pr.used;
            if (pr.rc != GAMUT_HIP_OK) return set_error(pr.rc, "%s", pr.msg);
            return GAMUT_HIP_OK;
        }
        std::vector<uint8_t> bytes(fp.rc == GAMUT_HIP_OK ? fp.cap : 0);
        if (fp.rc == GAMUT_HIP_OK) { fp.items.clear(); fp.dev_unstuff = false; unstuff_file(0, data, len, fp, bytes.data()); }   // (the host's walk: exact sizes)
        if (segments) *segments = (int32_t)fp.items.size();
        if (entropy_bytes) *entropy_bytes = fp.used;
        if (fp.rc != GAMUT_HIP_OK) return set_error(fp.rc, "%s", fp.msg);
        return GAMUT_HIP_OK;
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg_scan_layout: out of host memory");
    }
}

int gamut_hip_jpeg_entropy_decode_device(const uint8_t* const* data, const size_t* len, int count,
                                         const int64_t* coeff_offset, const int64_t* zag_offset,
                                         int16_t* coeffs, uint8_t* max_zag, uint32_t* status_dev,
                                         gamut_hip_jpeg_frame* info, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!data || !len || !coeff_offset || !zag_offset || !coeffs || !max_zag || !info)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "jpeg_entropy_decode_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {                                                      // std::vector / bad_alloc must not escape a C entry point
        return entropy_decode_device(data, len, count, coeff_offset, zag_offset, coeffs, max_zag, status_dev, info, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg_entropy_decode_device: out of host memory");
    }
}

int gamut_hip_jpeg_decode_batch_device(const uint8_t* const* data, const size_t* len, int count, int req_comps,
                                       const int64_t* out_offset, uint8_t* out, gamut_hip_jpeg_frame* info, int* status_host,
                                       uint32_t* status_dev, void* stream)
{
    clear_error();
    if (count < 0 || (req_comps != 1 && req_comps != 3 && req_comps != 4) || (count > 0 && (!data || !len || !out_offset || !out || !info)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "jpeg_decode_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        hipStream_t st = pick_stream(stream);
        static thread_local PerDevice<DeviceScratch> co_pd, zz_pd, tok_pd, strip_pd, offs_pd;
        DeviceScratch& s_co = co_pd.cur(); DeviceScratch& s_zz = zz_pd.cur();
        std::vector<int64_t> co_off((size_t)count, 0), zz_off((size_t)count, 0), tk_off((size_t)count, 0), sp_off((size_t)count, 0);
        std::vector<char> ok((size_t)count, 0), prog((size_t)count, 0), tokm((size_t)count, 0);
        int16_t* d_co = nullptr; uint8_t* d_zz = nullptr;
        uint32_t* d_tok = nullptr; uint32_t* d_strip = nullptr; int64_t* d_offs = nullptr;      // d_offs: [count] token offsets, [count] strip-table offsets
        // the hand-off between the entropy kernels and the reconstruction: tokens (the default where an image can: 4:2:0, one long
        // segment) or the dense 128-byte blocks of the public coefficient-level entry point; GAMUT_HIP_JPEG_HANDOFF=dense forces the latter
        const char* ho_env = getenv("GAMUT_HIP_JPEG_HANDOFF");
        const bool want_tokens = !(ho_env && !strcmp(ho_env, "dense"));
        DecodeHooks hooks;
        hooks.layout = [&](const gamut_hip_jpeg_frame* f, const int* rc, const char* progressive, int64_t* coeff_offset, int64_t* zag_offset, int16_t** pco, uint8_t** pzz,
                           const TokenPlan& plan) -> int {
            int64_t blocks = 0, zblocks = 0, tokens = 0, strips = 0;
            for (int i = 0; i < count; ++i) {
                coeff_offset[i] = blocks * 64; zag_offset[i] = zblocks;
                co_off[(size_t)i] = blocks * 64; zz_off[(size_t)i] = zblocks;
                ok[(size_t)i] = rc[i] == GAMUT_HIP_OK; prog[(size_t)i] = progressive[i];
                if (!ok[(size_t)i]) continue;
                const int64_t nblk = (int64_t)f[i].mcus_per_row * f[i].mcus_per_col * f[i].blocks_per_mcu;
                zblocks += nblk;
                // a token per DC and per non-zero AC coefficient: at most 64 per block, and no more than the scan has bit pairs plus a
                // DC token per block (a token costs two bits of the scan at least, a DC token of a block that ends at once one)
                const int64_t cap = std::min<int64_t>(nblk * 64, (int64_t)plan.scan_len[i] * 4 + nblk) + 16;
                // (the token kernel stores whole rgba8 pixels as dwords: an image whose rows would not be dword-aligned keeps the dense hand-off, whose
                //  launch falls back to the byte-wise kernel -- jpeg_reconstruct_launch)
                const bool dword_rows = req_comps != 4 || ((((uintptr_t)out + (uint64_t)out_offset[i]) & 3) == 0);
                if (want_tokens && plan.tok_ok[i] && cap < 0x7fffffff && dword_rows) {
                    tokm[(size_t)i] = 1; plan.tok[i] = 1;
                    tk_off[(size_t)i] = tokens; plan.tok_off[i] = tokens; plan.tok_cap[i] = (int32_t)cap;
                    sp_off[(size_t)i] = strips; plan.strip_off[i] = strips;
                    tokens += (cap + 3) & ~(int64_t)3;
                    strips += (int64_t)f[i].mcus_per_col * ((f[i].mcus_per_row + 7) / 8) + 1;
                } else blocks += nblk;
            }
            d_co = (int16_t*)s_co.get((size_t)blocks * 128 + 256, st); d_zz = (uint8_t*)s_zz.get((size_t)zblocks + 256, st);
            if (!d_co || !d_zz) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg_decode_batch_device: %lld coefficient blocks do not fit the device", (long long)blocks);
            *pco = d_co; *pzz = d_zz;
            if (tokens) {
                d_tok = (uint32_t*)tok_pd.cur().get((size_t)tokens * 4 + 256, st);
                d_strip = (uint32_t*)strip_pd.cur().get((size_t)strips * 4 + 256, st);
                d_offs = (int64_t*)offs_pd.cur().get((size_t)count * 16 + 256, st);
                if (!d_tok || !d_strip || !d_offs) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg_decode_batch_device: %lld tokens do not fit the device", (long long)tokens);
                *plan.d_tokens = d_tok; *plan.d_strip_tab = d_strip;
                // (pageable sources: the runtime has read them when the calls return; the kernels that use the table are queued later)
                GAMUT_HIP_CHECK(hipMemcpyAsync(d_offs, tk_off.data(), (size_t)count * 8, hipMemcpyHostToDevice, st));
                GAMUT_HIP_CHECK(hipMemcpyAsync(d_offs + count, sp_off.data(), (size_t)count * 8, hipMemcpyHostToDevice, st));
            }
            return GAMUT_HIP_OK;
        };
        // images [lo, hi) -> pixels: runs of images of one geometry (and one kind of hand-off) at even strides go out as one batched launch
        auto reconstruct = [&](int lo, int hi, hipStream_t gs, bool progressive_only) -> int {
            for (int i = lo; i < hi; ) {
                const gamut_hip_jpeg_frame& f = info[i];
                const bool mine = ok[(size_t)i] && (prog[(size_t)i] != 0) == progressive_only;
                if (!mine) { ++i; continue; }
                const int64_t nblk = (int64_t)f.mcus_per_row * f.mcus_per_col * f.blocks_per_mcu;
                const bool tk = tokm[(size_t)i] != 0;
                int j = i + 1;
                const int64_t ostride = j < hi ? out_offset[j] - out_offset[i] : 0;
                while (j < hi && ok[(size_t)j] && (prog[(size_t)j] != 0) == progressive_only && (tokm[(size_t)j] != 0) == tk && info[j].width == f.width && info[j].height == f.height &&
                       info[j].scan_type == f.scan_type && (tk || co_off[(size_t)j] - co_off[(size_t)j - 1] == nblk * 64) && zz_off[(size_t)j] - zz_off[(size_t)j - 1] == nblk &&
                       out_offset[j] - out_offset[j - 1] == ostride && ostride > 0) ++j;
                if (tk) {
                    if (int rc = jpeg_reconstruct_tokens_launch(d_tok, d_strip, d_offs + i, d_offs + count + i, d_zz + zz_off[(size_t)i], nblk, out + out_offset[i],
                                                                (int64_t)f.width * req_comps, j - i > 1 ? ostride : 0, f.width, f.height, req_comps, j - i, gs)) return rc;
                } else
                if (int rc = jpeg_reconstruct_launch(d_co + co_off[(size_t)i], nblk * 64, d_zz + zz_off[(size_t)i], nblk, out + out_offset[i], (int64_t)f.width * req_comps,
                                                     j - i > 1 ? ostride : 0, f.width, f.height, f.scan_type, req_comps, j - i, gs)) return rc;
                i = j;
            }
            return GAMUT_HIP_OK;
        };
        hooks.group_done = [&](int lo, int hi, hipStream_t gs) -> int { return reconstruct(lo, hi, gs, false); };
        // a baseline file the host feeder decoded behind the device pass (kHostRedo): its coefficients go up and through the dense reconstruction
        hooks.redo = [&](int i, const gamut_hip_jpeg_frame& fr, hipStream_t s) -> int {
            StreamDrain drain; drain.arm(s);                   // (pageable sources, freed when host_redo returns)
            if (int rc = reconstruct_host_frame(fr, out + out_offset[i], req_comps, s)) return rc;
            if (drain.wait() != hipSuccess) return set_error(GAMUT_HIP_ERR_HIP, "jpeg_decode_batch_device: reconstruction of image %d failed", i);
            return GAMUT_HIP_OK;
        };
        // per-file verdicts: the header-level ones (host) and what the kernels flag (device) are folded into ONE status per file, as
        // gamut_hip_png_decode_batch_device does -- a caller that passes no status arrays still gets the failure as the return value
        std::vector<int> own_host; int* hst = status_host;
        if (!hst) { own_host.assign((size_t)count, GAMUT_HIP_OK); hst = own_host.data(); }
        static thread_local PerDevice<DeviceScratch> st_pd;
        uint32_t* d_st = status_dev;
        if (!d_st) { d_st = (uint32_t*)st_pd.cur().get((size_t)count * sizeof(uint32_t), st); if (!d_st) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg_decode_batch_device: status allocation failed"); }
        int rc = entropy_decode_device(data, len, count, nullptr, nullptr, nullptr, nullptr, d_st, info, hst, st, &hooks);
        if (rc != GAMUT_HIP_OK && rc != GAMUT_HIP_ERR_DECODE && rc != GAMUT_HIP_ERR_UNSUPPORTED) return rc;     // not a per-file verdict: allocation / HIP failure
        char first_msg[200]; snprintf(first_msg, sizeof(first_msg), "%s", last_error_buf());
        // (entropy_decode_device returns when every stream it used has drained: the baseline files' pixels are in place.  The
        // progressive files' coefficients were decoded after the groups: their pixels follow here -- not those of a file whose scans
        // could not be prepared: its share of the coefficient scratch holds whatever an earlier batch left there.)
        if (d_co) {
            for (int i = 0; i < count; ++i) if (prog[(size_t)i] && hst[i] != GAMUT_HIP_OK) ok[(size_t)i] = 0;
            std::vector<uint32_t> flags((size_t)count);
            StreamDrain drain; drain.arm(st);                   // the per-thread coefficient scratch is reused by the next call: every way out from here waits for `st`
            if (int rc2 = reconstruct(0, count, st, true)) return rc2;
            GAMUT_HIP_CHECK(hipMemcpyAsync(flags.data(), d_st, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            GAMUT_HIP_CHECK(drain.wait());
            int first = -1;
            for (int i = 0; i < count; ++i) {
                if (hst[i] == GAMUT_HIP_OK && flags[(size_t)i]) {       // a damaged entropy-coded segment: the file's pixels are what the decode of the damage gives
                    hst[i] = GAMUT_HIP_ERR_DECODE;
                    if (first < 0) first = i;
                }
            }
            int lowest = -1;
            for (int i = 0; i < count; ++i) if (hst[i] != GAMUT_HIP_OK) { lowest = i; break; }
            if (lowest >= 0 && lowest == first) return set_error(GAMUT_HIP_ERR_DECODE, "image %d: corrupt entropy-coded data", first);
            if (lowest >= 0) return set_error(hst[lowest], "%s", first_msg[0] ? first_msg : "jpeg_decode_batch_device: a file failed");
        }
        if (rc != GAMUT_HIP_OK) return set_error(rc, "%s", first_msg);
        return GAMUT_HIP_OK;
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "jpeg_decode_batch_device: out of host memory");
    }
}

void gamut_hip_jpeg_frame_free(gamut_hip_jpeg_frame* f)
{
    if (!f) return;
    free(f->coeffs); free(f->max_zag);
    f->coeffs = nullptr; f->max_zag = nullptr;
}

int gamut_hip_jpeg_reconstruct_batch_device(const int16_t* coeffs, int64_t coeff_stride,
                                            const uint8_t* max_zag, int64_t zag_stride,
                                            uint8_t* out, int64_t out_pitch, int64_t out_stride,
                                            int width, int height, int scan_type, int out_comps,
                                            int count, void* stream)
{
    clear_error();
    return jpeg_reconstruct_launch(coeffs, coeff_stride, max_zag, zag_stride, out, out_pitch, out_stride,
                                   width, height, scan_type, out_comps, count, pick_stream(stream));
}

int gamut_hip_jpeg_reconstruct_device(const gamut_hip_jpeg_desc* descs, int count, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && !descs)) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "jpeg_reconstruct: bad descriptor array");
    hipStream_t st = pick_stream(stream);
    for (int i = 0; i < count; ++i) {
        const gamut_hip_jpeg_desc& d = descs[i];
        if (int rc = jpeg_reconstruct_launch(d.coeffs, 0, d.max_zag, 0, d.out, d.out_pitch, 0,
                                             d.width, d.height, d.scan_type, d.out_comps, 1, st))
            return rc;
    }
    return GAMUT_HIP_OK;
}

// decompress_jpeg_image_from_stream (jpegload.d:3720-3808) on a memory buffer
uint8_t* gamut_hip_decompress_jpeg_image_from_memory(const uint8_t* data, size_t len,
        int* width, int* height, int* actual_comps, float* pixelAspectRatio, float* dotsPerInchY, int req_comps)
{
    clear_error();
    if (req_comps != -1 && req_comps != 1 && req_comps != 3 && req_comps != 4) {          // :3727
        set_error(GAMUT_HIP_ERR_INVALID_ARG, "decompress_jpeg: req_comps must be -1, 1, 3 or 4");
        return nullptr;
    }
    gamut_hip_jpeg_frame f;
    if (decode_coeffs(data, len, &f)) return nullptr;
    if (width) *width = f.width;
    if (height) *height = f.height;
    if (actual_comps) *actual_comps = f.comps;
    if (pixelAspectRatio) *pixelAspectRatio = -1;
    if (dotsPerInchY) *dotsPerInchY = -1;
    if (req_comps < 0) req_comps = f.comps;

    const size_t dst_bpl = (size_t)f.width * req_comps, out_bytes = dst_bpl * f.height;
    uint8_t* result = (uint8_t*)malloc(out_bytes ? out_bytes : 1);                          // :3749, free()-compatible
    void* dout = nullptr;
    hipStream_t st = thread_stream();
    bool ok = result != nullptr;
    if (!ok) set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "decompress_jpeg: out of memory");
    auto hip_ok = [&](hipError_t e, const char* what) {
        if (e != hipSuccess) { set_error(GAMUT_HIP_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e)); return false; }
        return true;
    };
    // device staging of the call: per-thread buffers that grow and stay (a hipMalloc / hipFree pair per buffer and call cost more than
    // the decode of a small image)
    static thread_local PerDevice<DeviceScratch> s_out_pd;
    if (ok) {
        dout = s_out_pd.cur().get(out_bytes + 16);
        if (!dout) { set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "decompress_jpeg: device staging allocation failed"); ok = false; }
    }
    ok = ok && reconstruct_host_frame(f, (uint8_t*)dout, req_comps, st) == GAMUT_HIP_OK;
    ok = ok && hip_ok(hipMemcpyAsync(result, dout, out_bytes, hipMemcpyDeviceToHost, st), "hipMemcpyAsync") &&
         hip_ok(hipStreamSynchronize(st), "hipStreamSynchronize");
    if (ok) {
        if (pixelAspectRatio) *pixelAspectRatio = f.pixel_aspect_ratio;                     // :3804-3805
        if (dotsPerInchY) *dotsPerInchY = f.dpi_y;
    } else { free(result); result = nullptr; }
    gamut_hip_jpeg_frame_free(&f);
    return result;
}

} // extern "C"
