// gif_encode_host.hip -- GIF encode: arguments, the batch's tables and the entry points; the kernels are in gif_encode.hip.
//
// What a file is (msf_gif.d): the 32-byte header with the NETSCAPE2.0 loop block (:545-548), one block per frame -- GCE and image
// descriptor (18 bytes, :408-418), a local colour table of 1 << tableBits entries, the LZW minimum code size, the code stream in
// 255-byte sub-blocks, a zero terminator -- and 0x3B.  saveGIF (plugins/gif.d:105-147) makes every layer of an rgba8 image a frame of
// 7 centiseconds at maxBitDepth 16 with the alpha threshold 10 (the struct default, msf_gif.d:123); the batch entry takes the three as
// arguments.  maxBitDepth is clamped to 1..16 (:573); the delay is written with its low 16 bits (:414).
//
// DELIBERATE DEVIATIONS from the reference:
//   * a width or height below 1 or above 65535 (the reference writes truncated 16-bit fields and a file no reader takes for the
//     image): refused;
//   * frames < 1 (saveGIF :116): refused, as there;
//   * a shape with width * height * 4 > INT_MAX (the reference's int sizes, :337-346 and :530, wrap): refused.
#include "gif_encode_host.hpp"
#include "encode_host.hpp"

namespace gamut {

int64_t gifenc_frame_reservation(int w, int h) { return 32 + 768 + (int64_t)w * h * 3 / 2 + 256; }        // :337-345

int64_t gifenc_bound(int w, int h, int frames)
{
    if (w < 1 || h < 1 || w > 65535 || h > 65535 || frames < 1 || (int64_t)w * h * 4 > 0x7fffffffLL) return 0;
    return 32 + (int64_t)frames * gifenc_frame_reservation(w, h) + 1;
}

GifEncMul gifenc_mul_table()
{
    GifEncMul m{ 0 };
    for (int bits = 0; bits <= 6; ++bits) {
        const int diff = (1 << (8 - bits)) - 1;
        const short mul = (short)((255.0f - diff) / 255.0f * 257);                                           // :214-216, as written there
        m.packed |= (uint64_t)(uint16_t)mul << (9 * bits);
    }
    return m;
}

namespace {

// Measurements (tools/gif_encode_bench.py): with GAMUT_HIP_GIF_TIMING=1 the encode call brackets each of its five kernels with events
// and keeps the GPU times of the calling thread's last call: census, plan, LZW, offsets, gather.
thread_local float t_last_ms[5] = { -1.0f, -1.0f, -1.0f, -1.0f, -1.0f };

int encode_batch(const uint8_t* const* src, const int64_t* src_pitch, const int64_t* src_layer_offset, const int32_t* width, const int32_t* height,
                 const int32_t* frames, const int32_t* centiseconds, const int32_t* max_bit_depth, const int32_t* alpha_threshold, int count,
                 const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host, hipStream_t stream)
{
    std::vector<GifEncAnim> anims; std::vector<GifEncFrame> fr; std::vector<int> which;
    int first_bad = -1, first_outgrown = -1;
    uint64_t census_units = 0, gather_units = 0, slot_bytes = 0;
    for (int i = 0; i < count; ++i) {
        out_len[i] = 0;
        const bool ok = gifenc_bound(width[i], height[i], frames[i]) > 0 && src[i] && out_offset[i] >= 0;
        if (status_host) status_host[i] = ok ? GAMUT_HIP_OK : GAMUT_HIP_ERR_INVALID_ARG;
        if (!ok) { if (first_bad < 0) first_bad = i; continue; }
        GifEncAnim a{};
        a.src = src[i]; a.pitch = src_pitch[i]; a.layer_off = src_layer_offset[i]; a.out_off = out_offset[i];
        a.w = (uint32_t)width[i]; a.h = (uint32_t)height[i]; a.frames = (uint32_t)frames[i]; a.frame0 = (uint32_t)fr.size();
        a.centis = centiseconds ? centiseconds[i] : 7;
        a.max_depth = std::max(1, std::min(16, max_bit_depth ? max_bit_depth[i] : 16));                     // :573
        a.alpha_thr = alpha_threshold ? alpha_threshold[i] : 10;
        a.aligned = (((uintptr_t)a.src | (uint64_t)a.pitch | (uint64_t)a.layer_off) & 3u) == 0 ? 1u : 0u;
        const uint64_t npx = (uint64_t)a.w * a.h;
        const uint64_t cap = (uint64_t)gifenc_frame_reservation(width[i], height[i]);      // what a block may take, as in the reference
        const uint64_t stride = (cap + 3 + 3) & ~(uint64_t)3;                               // (the block starts up to 3 bytes into its slot)
        const uint32_t cu = (uint32_t)((npx + kGifCensusPixels - 1) / kGifCensusPixels), gu = (uint32_t)((cap + kGifGatherBytes - 1) / kGifGatherBytes);
        for (uint32_t f = 0; f < a.frames; ++f) {
            GifEncFrame e{};
            e.slot = slot_bytes; e.slot_cap = (uint32_t)cap; e.anim = (uint32_t)anims.size(); e.index = f;
            e.census0 = (uint32_t)census_units; e.gather0 = (uint32_t)gather_units;
            slot_bytes += stride; census_units += cu; gather_units += gu;
            if (census_units > 0x7FFFFFFFull || gather_units > 0x7FFFFFFFull || fr.size() >= 0x7FFFFFFFull)
                return set_error(GAMUT_HIP_ERR_INVALID_ARG, "gif_encode: batch of more than 2^31 units");
            fr.push_back(e);
        }
        anims.push_back(a); which.push_back(i);
    }
    if (!anims.empty()) {
        const int n = (int)anims.size(); const size_t nfr = fr.size();
        // uploaded: animations, frames.  device only: plans, lengths, transparent flags, bitmaps (the last two zeroed by one memset)
        const size_t o_anim = 0, o_fr = up256((size_t)n * sizeof(GifEncAnim)), o_up_end = o_fr + up256(nfr * sizeof(GifEncFrame));
        const size_t o_plan = o_up_end, o_len = o_plan + up256(nfr * sizeof(GifEncPlan)), o_tr = o_len + up256((size_t)n * 8),
                     o_bm = o_tr + up256(nfr * 4), total = o_bm + up256(nfr * (size_t)kGifCensusWords * 4);
        static thread_local PerDevice<DeviceScratch> scratch_pd, slot_pd;
        static thread_local PerDevice<PinnedScratch> pinned_pd;
        uint8_t* d = (uint8_t*)scratch_pd.cur().get(total, stream);
        uint8_t* dslots = (uint8_t*)slot_pd.cur().get((size_t)slot_bytes + 16, stream);
        uint8_t* h = pinned_pd.cur().get(o_up_end + (size_t)n * 8, stream);
        if (!d || !dslots || !h) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "gif_encode: scratch of %zu + %llu bytes failed", total, (unsigned long long)slot_bytes);
        memcpy(h + o_anim, anims.data(), (size_t)n * sizeof(GifEncAnim));
        memcpy(h + o_fr, fr.data(), nfr * sizeof(GifEncFrame));
        GAMUT_HIP_CHECK(hipMemcpyAsync(d, h, o_up_end, hipMemcpyHostToDevice, stream));
        GAMUT_HIP_CHECK(hipMemsetAsync(d + o_tr, 0, total - o_tr, stream));
        static const bool timing = env_flag("GAMUT_HIP_GIF_TIMING");
        KernelTimer<6> timer(timing);
        for (float& t : t_last_ms) t = -1.0f;
        int64_t* dlen = (int64_t*)(d + o_len);
        if (int rc = gifenc_launch((const GifEncAnim*)(d + o_anim), n, (const GifEncFrame*)(d + o_fr), (uint32_t)nfr, (uint32_t)census_units,
                                   (uint32_t)gather_units, (uint32_t*)(d + o_bm), (uint32_t*)(d + o_tr), (GifEncPlan*)(d + o_plan), dslots, dlen, out,
                                   gifenc_mul_table(), stream, timer)) return rc;
        int64_t* hlen = (int64_t*)(h + o_up_end);
        GAMUT_HIP_CHECK(hipMemcpyAsync(hlen, dlen, (size_t)n * 8, hipMemcpyDeviceToHost, stream));
        GAMUT_HIP_CHECK(hipStreamSynchronize(stream));
        timer.finish(t_last_ms);
        for (int k = 0; k < n; ++k) {
            const int i = which[(size_t)k];
            if (hlen[k] > 0) { out_len[i] = hlen[k]; continue; }
            if (status_host) status_host[i] = GAMUT_HIP_ERR_HIP;      // a block outgrew the reference's reservation: cannot happen
            if (first_outgrown < 0) first_outgrown = i;
        }
    }
    // the status of the lowest-numbered animation that has one
    if (first_outgrown >= 0 && (first_bad < 0 || first_outgrown < first_bad))
        return set_error(GAMUT_HIP_ERR_HIP, "image %d: gif_encode: a frame outgrew its reservation", first_outgrown);
    if (first_bad >= 0) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "image %d: gif_encode: refused shape, frame count or source", first_bad);
    return GAMUT_HIP_OK;
}

} // namespace
} // namespace gamut

using namespace gamut;

extern "C" {

int64_t gamut_hip_gif_encode_bound(int width, int height, int frames) { return gifenc_bound(width, height, frames); }

int gamut_hip_gif_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const int64_t* src_layer_offset, const int32_t* width,
                                      const int32_t* height, const int32_t* frames, const int32_t* centiseconds, const int32_t* max_bit_depth,
                                      const int32_t* alpha_threshold, int count, const int64_t* out_offset, uint8_t* out, int64_t* out_len,
                                      int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!src || !src_pitch || !src_layer_offset || !width || !height || !frames || !out_offset || !out || !out_len)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "gif_encode_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return encode_batch(src, src_pitch, src_layer_offset, width, height, frames, centiseconds, max_bit_depth, alpha_threshold, count, out_offset,
                            out, out_len, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "gif_encode_batch_device: out of host memory");
    }
}

void* gamut_hip_gif_write_to_mem(const void* data, int pitch, int64_t layer_offset, int w, int h, int frames, int centiseconds, int max_bit_depth,
                                 int alpha_threshold, int* out_len)
{
    clear_error();
    const int64_t bound64 = gifenc_bound(w, h, frames);
    if (!data || !out_len || bound64 == 0 || bound64 > 0x7fffffffLL || (int64_t)w * h * 4 * frames > 0x7fffffffLL) {   // (the length is handed back through an int)
        set_error(GAMUT_HIP_ERR_INVALID_ARG, "gif_write_to_mem: invalid arguments"); return nullptr;
    }
    if (!have_device()) return nullptr;
    const int32_t W = w, H = h, F = frames, CS = centiseconds, MD = max_bit_depth, AT = alpha_threshold;
    return encode_host_image("gif_write_to_mem", HostRows{ data, pitch, (size_t)w * 4, h, frames, layer_offset }, (size_t)bound64, out_len,
        [&](const uint8_t* src, int64_t spitch, int64_t slayer, int64_t off, uint8_t* d, int64_t* n, hipStream_t st) {
            int status = 0;
            return encode_batch(&src, &spitch, &slayer, &W, &H, &F, &CS, &MD, &AT, 1, &off, d, n, &status, st);
        });
}

float gamut_hip_gif_last_encode_kernel_ms(int which) { return which >= 0 && which < 5 ? t_last_ms[which] : -1.0f; }

} // extern "C"
