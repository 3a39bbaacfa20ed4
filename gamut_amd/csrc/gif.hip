// gif.hip -- GIF on the GPU: the frames of GIFDecoder.decodeNextFrame (source/gamut/codecs/gif.d), composited as loadGIF
// (source/gamut/plugins/gif.d:57-103) leaves them in a layered rgba8 image, many files per call.  The container is walked on the host
// (gif_host.hip, which also lists the deliberate deviations); two kernels do the rest.
//
// k_gif_lzw -- one frame per WAVE (a workgroup of 64 lanes), every frame of every file of the batch in one launch.  LZW is a serial
// chain per frame and the frames are independent, so the parallelism is across frames; within a frame the lanes share the one thing
// that is wide, the string copy.  A new table entry is always "the string just written plus the first byte of the next one", so an
// entry is kept as (position in the already decoded output, length) instead of a prefix chain: emitting a code is a copy from the
// frame's own index buffer that the lanes do together, 64 bytes per step, and KwKwK (code == the entry being made) is the previous
// string plus its own first byte.  One wave and not a wider workgroup: the code walk is scalar work that more waves would only wait
// for, lanes of ONE wave see each other's global stores in issue order without a fence or a barrier (the copy source may have been
// written by the previous code: LLVM's AMDGPUUsage, "Memory Model", gfx90a / gfx942 and later -- the vector memory operations of a
// wavefront are issued and completed in order through one L1, so wavefront-scope ordering needs no cache action or wait, only the
// compiler-level fence the loop carries), and the table -- 4096 x (u32, u16), codes above 4095 can only be read back for lzw_cs 12, whose
// entries 4098..8191 fold onto 2..4095 -- is 24 KiB of LDS, so six frames decode per CU at once.
// The payload is fetched 256 bytes at a time (a dword per lane, the next chunk requested while the current one is used) and handed
// out by v_readlane.  Indices that can no longer land on the screen (position >= rows * width, gif_host.hip) are not stored, but
// their codes are walked to the end: they decide the verdict.  Every loop consumes payload bits, loads are guarded by the payload's
// length and stores by the frame's index count, so a damaged stream neither reads nor writes outside its own buffers.
//
// k_gif_compose -- a thread per screen pixel; it walks its file's frames in order with output pixel, background pixel and history
// bit in registers (disposal, parseFrame :364-410; the pixel rule of stbi__out_gif_code :789-799), fetches the frame's index through
// the row order and the frame's palette snapshot, and stores the pixel to that frame's layer: a wave stores 256 consecutive bytes.
// Files with a refused frame are left untouched.
#include "gif_host.hpp"
#include "device_util.hpp"
#include <string>

namespace gamut {
namespace {

constexpr int kWave = 64;
constexpr int kComposeThreads = 256;
constexpr uint32_t kPosSat = 0x7FFFFFFFu;

struct DFrame {
    uint64_t payload;                // byte offset in the blob, a multiple of 4; zero bytes up to the next multiple of 4 behind payload_len
    uint64_t idx;                    // byte offset of the frame's indices in the index scratch
    int64_t  rowmap;                 // offset in the row maps, -1: stream row = y - fy
    uint32_t payload_len;
    uint32_t limit;                  // rows * fw: indices worth keeping
    int32_t  fx, fy, fw, rows;
    int32_t  dispose, pal, lzw_cs, file;
};
struct DFile {
    int64_t  out_off;
    uint32_t w, h, frame0, nframes;
    uint32_t unit0, units;
};

__global__ void __launch_bounds__(kWave)
k_gif_lzw(const DFrame* __restrict__ frames, const uint8_t* __restrict__ blob, uint8_t* idx_all, uint32_t* frame_count, uint32_t* file_bad)
{
    __shared__ uint32_t tab_pos[4096];
    __shared__ uint16_t tab_len[4096];
    const DFrame& fr = frames[blockIdx.x];
    const int lane = threadIdx.x;
    const uint8_t* payload = blob + fr.payload;
    uint8_t* idx = idx_all + fr.idx;
    const uint32_t limit = fr.limit, plen = fr.payload_len;
    const uint32_t ndw = (plen + 3) >> 2;                            // dwords of payload (the last one padded with zeros in the blob)
    const uint64_t total_bits = (uint64_t)plen * 8;
    const int lzw_cs = fr.lzw_cs;
    const int clear = 1 << lzw_cs, maxcode = lzw_cs == 12 ? 8191 : 4095;

    auto load_chunk = [&](uint32_t chunk) -> uint32_t {              // dword chunk * 64 + lane of the payload, 0 behind its end
        const uint32_t d = chunk * kWave + lane;
        return d < ndw ? reinterpret_cast<const uint32_t*>(payload)[d] : 0u;
    };
    uint32_t chunk_cur = load_chunk(0), chunk_nxt = load_chunk(1);
    uint32_t next_dw = 0;                                            // the next dword to hand out
    uint64_t buf = 0, used = 0; int nb = 0;

    int codesize = lzw_cs + 1, codemask = (1 << codesize) - 1, avail = clear + 2;
    bool first = true, have_old = false, bad = false;
    uint32_t cur = 0, prev_pos = 0, prev_len = 0;

    while (used + (uint64_t)codesize <= total_bits) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");               // (compiler order only: one wave's LDS and global accesses are served in issue order)
        if (nb < codesize) {
            const int l = (int)(next_dw & (kWave - 1));
            if (l == 0 && next_dw != 0) { chunk_cur = chunk_nxt; chunk_nxt = load_chunk((next_dw >> 6) + 1); }
            const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)chunk_cur, l);
            buf |= (uint64_t)w << nb; nb += 32; ++next_dw;
        }
        const int code = (int)(buf & (uint64_t)codemask);
        buf >>= codesize; nb -= codesize; used += (uint64_t)codesize;
        if (code == clear) { codesize = lzw_cs + 1; codemask = (1 << codesize) - 1; avail = clear + 2; have_old = false; first = false; continue; }
        if (code == clear + 1) break;                               // end code: what follows in the chain is skipped (the host checked that it is all there)
        if (code > avail || first) { bad = true; break; }           // illegal code / no clear code in front of the first data code
        bool kwk = false;
        if (have_old) {
            const int a = avail++;
            if (avail > 8192) { bad = true; break; }                 // too many codes
            if (a <= maxcode && lane == 0) { tab_pos[a & 4095] = prev_pos; tab_len[a & 4095] = (uint16_t)(prev_len + 1); }
            kwk = code == a;
        } else if (code == avail) { bad = true; break; }
        uint32_t src = 0, len = 1;
        const bool literal = code < clear;
        if (kwk) { src = prev_pos; len = prev_len + 1; }
        else if (!literal) {
            src = (uint32_t)__builtin_amdgcn_readfirstlane((int)tab_pos[code & 4095]);
            len = (uint32_t)__builtin_amdgcn_readfirstlane((int)tab_len[code & 4095]);
        }
        if (cur < limit) {
            if (literal) { if (lane == 0) idx[cur] = (uint8_t)code; }
            else {
                if (src >= cur) { bad = true; break; }                       // (cannot happen: an entry lies in front of the write position)
                for (uint32_t k0 = 0; k0 < len && cur + k0 < limit; k0 += kWave) {
                    const uint32_t k = k0 + lane;
                    if (k < len && cur + k < limit) idx[cur + k] = idx[src + ((kwk && k == len - 1) ? 0u : k)];
                }
            }
        }
        prev_pos = cur; prev_len = len;
        cur = cur + len < kPosSat ? cur + len : kPosSat;
        if ((avail & codemask) == 0 && avail <= 0x0FFF) { ++codesize; codemask = (1 << codesize) - 1; }
        have_old = true;
    }
    if (lane == 0) {
        frame_count[blockIdx.x] = cur < limit ? cur : limit;
        if (bad) atomicOr(&file_bad[fr.file], 1u);
    }
}

__global__ void __launch_bounds__(kComposeThreads)
k_gif_compose(const DFile* __restrict__ files, int nfiles, const DFrame* __restrict__ frames, const uint8_t* __restrict__ idx_all,
              const uint32_t* __restrict__ frame_count, const uint32_t* __restrict__ file_bad, const uint32_t* __restrict__ palettes,
              const uint16_t* __restrict__ rowmaps, uint8_t* out)
{
    const int fi = find_unit<&DFile::unit0>(files, nfiles, blockIdx.x);
    const DFile& f = files[fi];
    if (file_bad[fi]) return;
    const uint64_t npx = (uint64_t)f.w * f.h;
    const uint64_t p = (uint64_t)(blockIdx.x - f.unit0) * kComposeThreads + threadIdx.x;
    if (p >= npx) return;
    const int y = (int)(p / f.w), x = (int)(p - (uint64_t)y * f.w);
    uint8_t* o = out + f.out_off + p * 4;
    const bool aligned = (reinterpret_cast<uintptr_t>(o) & 3) == 0;
    uint32_t px = 0, bg = 0; bool hist = false;
    for (uint32_t k = 0; k < f.nframes; ++k) {
        const DFrame& fr = frames[f.frame0 + k];
        if (k) { if (fr.dispose == 2 && hist) px = bg; bg = px; }
        const int dx = x - fr.fx;
        if (dx >= 0 && dx < fr.fw) {
            int r = -1;
            if (fr.rowmap < 0) r = y - fr.fy;
            else { const uint32_t m = rowmaps[fr.rowmap + y]; r = m == 0xFFFFu ? -1 : (int)m; }
            if (r >= 0 && r < fr.rows) {
                const uint32_t pos = (uint32_t)r * (uint32_t)fr.fw + (uint32_t)dx;
                if (pos < frame_count[f.frame0 + k]) {
                    hist = true;
                    const uint32_t c = palettes[(size_t)fr.pal * 256 + idx_all[fr.idx + pos]];       // bytes R G B A
                    if ((c >> 24) > 128u) px = c | 0xFF000000u;
                }
            }
        }
        if (aligned) *reinterpret_cast<uint32_t*>(o) = px;
        else { o[0] = (uint8_t)px; o[1] = (uint8_t)(px >> 8); o[2] = (uint8_t)(px >> 16); o[3] = (uint8_t)(px >> 24); }
        o += npx * 4;
    }
}

// Measurements (tools/gif_bench.py): with GAMUT_HIP_GIF_TIMING=1 the decode call brackets each of its two kernels -- not the upload --
// with events and keeps the GPU times of the calling thread's last call.
thread_local float t_last_ms[2] = { -1.0f, -1.0f };

int decode_batch(const uint8_t* const* data, const size_t* len, int count, const int64_t* out_offset, const int64_t* out_capacity, uint8_t* out,
                 gamut_hip_gif_info* info, int* status_host, hipStream_t stream, bool& per_file)
{
    std::vector<GifParsed> parsed((size_t)count);
    std::vector<gamut_hip_gif_info> infos((size_t)count);
    std::vector<int> rcs((size_t)count);
    std::vector<std::string> msgs((size_t)count);
    parallel_for(count, std::min(host_threads(), count), [&](int, int i) {
        try {
            rcs[(size_t)i] = gif_parse(data[i], len[i], false, &parsed[(size_t)i], &infos[(size_t)i]);
            const gamut_hip_gif_info& gi = infos[(size_t)i];
            if (rcs[(size_t)i] == GAMUT_HIP_OK && out_offset[i] < 0) rcs[(size_t)i] = set_error(GAMUT_HIP_ERR_INVALID_ARG, "gif: negative out_offset");
            if (rcs[(size_t)i] == GAMUT_HIP_OK && (int64_t)gi.layers * gi.width * gi.height * 4 > out_capacity[i])
                rcs[(size_t)i] = set_error(GAMUT_HIP_ERR_INVALID_ARG, "gif: %d layers of %d x %d do not fit out_capacity", gi.layers, gi.width, gi.height);
        } catch (...) { rcs[(size_t)i] = set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "gif: out of host memory"); }
        if (rcs[(size_t)i] != GAMUT_HIP_OK) msgs[(size_t)i] = last_error_buf();
    });
    // the batch's tables
    std::vector<DFile> files; std::vector<DFrame> frames; std::vector<int> which;
    size_t blob = 0, npal = 0, nmap = 0; uint64_t idx_bytes = 0, units = 0;
    for (int i = 0; i < count; ++i) {
        if (rcs[(size_t)i] != GAMUT_HIP_OK) continue;
        const GifParsed& g = parsed[(size_t)i];
        const gamut_hip_gif_info& gi = infos[(size_t)i];
        DFile f{};
        f.out_off = out_offset[i]; f.w = (uint32_t)gi.width; f.h = (uint32_t)gi.height;
        f.frame0 = (uint32_t)frames.size(); f.nframes = (uint32_t)g.frames.size();
        f.unit0 = (uint32_t)units;
        f.units = f.nframes ? (uint32_t)(((uint64_t)f.w * f.h + kComposeThreads - 1) / kComposeThreads) : 0u;
        units += f.units;
        for (const GifFrame& s : g.frames) {
            DFrame d{};
            d.payload_len = (uint32_t)s.payload_len;
            d.limit = (uint32_t)((uint64_t)s.rows * (uint64_t)s.fw);
            d.idx = idx_bytes; idx_bytes += ((uint64_t)d.limit + 3) & ~(uint64_t)3;
            d.rowmap = s.rowmap < 0 ? -1 : (int64_t)nmap + s.rowmap;
            d.fx = s.fx; d.fy = s.fy; d.fw = s.fw; d.rows = s.rows; d.dispose = s.dispose; d.pal = (int32_t)(npal + (size_t)s.pal);
            d.lzw_cs = s.lzw_cs; d.file = (int32_t)files.size();
            if (s.payload_len > 0xFFFFFFF0ull) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "gif_decode: a frame of more than 4 GiB");
            frames.push_back(d);
        }
        // a frame's payload starts 4-aligned in the blob and is followed by zeros up to a multiple of 4
        size_t at = blob;
        for (size_t k = 0; k < g.frames.size(); ++k) { frames[f.frame0 + k].payload = at; at += (g.frames[k].payload_len + 3) & ~(size_t)3; }
        blob = at;
        npal += g.palettes.size() / 256; nmap += g.rowmaps.size();
        files.push_back(f); which.push_back(i);
    }
    if (units > 0x7FFFFFFFull || frames.size() > 0x7FFFFFFFull) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "gif_decode: batch of more than 2^31 units");
    std::vector<uint32_t> bad_host;
    if (!frames.empty()) {
        const int nf = (int)files.size(); const size_t nfr = frames.size();
        const size_t o_blob = 0, o_frames = up256(blob + 4), o_files = o_frames + up256(nfr * sizeof(DFrame)), o_pal = o_files + up256((size_t)nf * sizeof(DFile)),
                     o_map = o_pal + up256(npal * 1024), o_bad = o_map + up256(nmap * 2 + 2), o_cnt = o_bad + up256((size_t)nf * 4), total = o_cnt + up256(nfr * 4);
        static thread_local PerDevice<DeviceScratch> scratch_pd, idx_pd;
        static thread_local PerDevice<PinnedScratch> pinned_pd;
        uint8_t* d = (uint8_t*)scratch_pd.cur().get(total, stream);
        uint8_t* didx = (uint8_t*)idx_pd.cur().get((size_t)idx_bytes + 16, stream);
        uint8_t* h = pinned_pd.cur().get(total, stream);
        if (!d || !didx || !h) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "gif_decode: staging of %zu + %llu bytes failed", total, (unsigned long long)idx_bytes);
        size_t pal_at = 0, map_at = 0;
        for (int k = 0; k < nf; ++k) {
            const GifParsed& g = parsed[(size_t)which[(size_t)k]];
            for (size_t j = 0; j < g.frames.size(); ++j) {
                const DFrame& fr = frames[files[(size_t)k].frame0 + j];
                uint8_t* dst = h + o_blob + fr.payload;
                memcpy(dst, g.payload.data() + g.frames[j].payload_off, g.frames[j].payload_len);
                memset(dst + g.frames[j].payload_len, 0, (size_t)(((g.frames[j].payload_len + 3) & ~(size_t)3) - g.frames[j].payload_len));
            }
            memcpy(h + o_pal + pal_at * 4, g.palettes.data(), g.palettes.size() * 4); pal_at += g.palettes.size();
            memcpy(h + o_map + map_at * 2, g.rowmaps.data(), g.rowmaps.size() * 2); map_at += g.rowmaps.size();
        }
        memcpy(h + o_frames, frames.data(), nfr * sizeof(DFrame));
        memcpy(h + o_files, files.data(), (size_t)nf * sizeof(DFile));
        memset(h + o_bad, 0, (size_t)nf * 4);
        GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, o_cnt, hipMemcpyHostToDevice, stream));
        const DFrame* dfr = (const DFrame*)(d + o_frames);
        uint32_t* dbad = (uint32_t*)(d + o_bad); uint32_t* dcnt = (uint32_t*)(d + o_cnt);
        static const bool timing = env_flag("GAMUT_HIP_GIF_TIMING");
        KernelTimer<3> timer(timing);
        timer.mark(stream);
        hipLaunchKernelGGL(k_gif_lzw, dim3((uint32_t)nfr), dim3(kWave), 0, stream, dfr, d + o_blob, didx, dcnt, dbad);
        if (int rc = launch_status("gif_lzw")) return rc;
        timer.mark(stream);
        if (units) {
            hipLaunchKernelGGL(k_gif_compose, dim3((uint32_t)units), dim3(kComposeThreads), 0, stream, (const DFile*)(d + o_files), nf, dfr, didx, dcnt,
                               dbad, (const uint32_t*)(d + o_pal), (const uint16_t*)(d + o_map), out);
            if (int rc = launch_status("gif_compose")) return rc;
        }
        timer.mark(stream);
        GAMUT_HIP_CHECK(hipMemcpyAsync(h + o_bad, dbad, (size_t)nf * 4, hipMemcpyDeviceToHost, stream));
        GAMUT_HIP_CHECK(hipStreamSynchronize(stream));
        timer.finish(t_last_ms);
        bad_host.assign((const uint32_t*)(h + o_bad), (const uint32_t*)(h + o_bad) + nf);
        for (int k = 0; k < nf; ++k)
            if (bad_host[(size_t)k]) { rcs[(size_t)which[(size_t)k]] = GAMUT_HIP_ERR_DECODE; msgs[(size_t)which[(size_t)k]] = "gif: corrupt raster data"; }
    }
    int first_bad = -1;
    per_file = true;
    for (int i = 0; i < count; ++i) {
        if (info) info[i] = infos[(size_t)i];
        if (status_host) status_host[i] = rcs[(size_t)i];
        if (rcs[(size_t)i] != GAMUT_HIP_OK) {
            if (info && rcs[(size_t)i] == GAMUT_HIP_ERR_DECODE) { memset(&info[i], 0, sizeof(info[i])); info[i].pixel_aspect_ratio = -1.0f; }
            if (first_bad < 0) first_bad = i;
        }
    }
    if (first_bad >= 0) return set_error(rcs[(size_t)first_bad], "image %d: %s", first_bad, msgs[(size_t)first_bad].c_str());
    return GAMUT_HIP_OK;
}

} // namespace
} // namespace gamut

using namespace gamut;

extern "C" {

int gamut_hip_gif_decode_batch_device(const uint8_t* const* data, const size_t* len, int count, const int64_t* out_offset, const int64_t* out_capacity,
                                      uint8_t* out, gamut_hip_gif_info* info, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!data || !len || !out_offset || !out_capacity || !out)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "gif_decode_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    bool per_file = false;                                             // did the call get as far as the per-file statuses?
    int rc;
    try {
        rc = decode_batch(data, len, count, out_offset, out_capacity, out, info, status_host, pick_stream(stream), per_file);
    } catch (...) {
        rc = set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "gif_decode_batch_device: out of host memory");
    }
    if (!per_file) {                                                   // the call failed as a whole: every file carries the call's status, no info
        for (int i = 0; i < count; ++i) {
            if (status_host) status_host[i] = rc;
            if (info) { memset(&info[i], 0, sizeof(info[i])); info[i].pixel_aspect_ratio = -1.0f; }
        }
    }
    return rc;
}

float gamut_hip_gif_last_decode_kernel_ms(void) { return t_last_ms[0] < 0 || t_last_ms[1] < 0 ? -1.0f : t_last_ms[0] + t_last_ms[1]; }
float gamut_hip_gif_last_kernel_ms(int which) { return which == 0 || which == 1 ? t_last_ms[which] : -1.0f; }

} // extern "C"
