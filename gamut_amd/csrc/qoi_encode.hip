// qoi_encode.hip -- QOI encode on the GPU: the bytes of qoi_encode (source/gamut/codecs/qoi.d:295-436), many images per batch.
//
// An image is cut into tiles of kTile consecutive pixels (row-major, runs and the index table carry across rows); one LANE walks one
// tile with the reference's own loop, its 64-slot index table in LDS ([slot][lane]: conflict-free whatever the slots).  What a tile
// needs from the tiles before it is (a) the previous pixel -- read from the image --, (b) the run counter and (c) the index table as
// the earlier pixels left it.  A pixel that repeats its predecessor never touches the table and every other pixel writes its slot,
// so (c) is "per slot, the last earlier NON-REPEAT pixel with that hash, else 0", and (b) is the trailing run length mod 62.
// Five plain launches, no workgroup ever waits for another (dispatch order is not guaranteed):
//   1. k_enc_summary : per tile, the table its own non-repeat pixels leave (values + presence mask), whether every pixel repeats its
//                      predecessor, the trailing run length;
//   2. k_enc_carry   : one wave per image walks its tiles in order, lane = slot: each tile's incoming table (written over the
//                      tile's summary values) and incoming run counter;
//   3. k_enc_walk<0> : the walk with the carry-in, counting the bytes of each tile;
//   4. k_enc_scan    : one workgroup per image: exclusive scan of the counts -> each tile's offset in the stream; header, padding
//                      and the stream length;
//   5. k_enc_walk<1> : the same walk again, writing the bytes (dword stores where the position allows).
// The input is read three times (1, 3, 5).  Scratch per tile: 64 table words + 16 bytes of summary + 12 bytes of carry / count /
// offset, about 300 B per 1024 pixels (0.6 MB per 1080p frame).
#include "encode_host.hpp"
#include "device_util.hpp"

namespace gamut {
namespace {

constexpr uint32_t kPixelsMax = 400000000u;                                // qoi.d:251 QOI_PIXELS_MAX
constexpr int kHeader = 14, kPadding = 8;                                    // :245, :268
constexpr int kTile = 1024;                                                  // pixels per tile (one lane's walk)
constexpr int kLanes = 64;                                                   // one wave per workgroup: LDS table of 16 KB
constexpr int kCarryAhead = 16;                                              // tiles whose summaries k_enc_carry loads before using them

struct EncImg {
    const uint8_t* src; int64_t pitch; int64_t out_off;
    uint32_t w, h, npx, ch, colorspace;
    uint32_t tile0, ntiles, pad;                                             // tiles [tile0, tile0 + ntiles) of the batch
};
struct TileMeta { uint32_t mask_lo, mask_hi, allrep, trail; };

__device__ __forceinline__ uint32_t enc_hash(uint32_t px) { return __builtin_amdgcn_udot4(px, 0x0B070503u, 0u, false) & 63u; }  // QOI_COLOR_HASH % 64

// pixel reader: rows of `pitch` bytes (negative allowed), any alignment; 3 channels get alpha 255 (qoi.d:356-366)
struct EncReader {
    const uint8_t* row; int64_t pitch; uint32_t x, w, ch;
    __device__ __forceinline__ void seek(const EncImg& im, uint32_t p)
    {
        const uint32_t y = p / im.w;
        x = p - y * im.w; w = im.w; ch = im.ch; pitch = im.pitch;
        row = im.src + (int64_t)y * im.pitch;
    }
    __device__ __forceinline__ uint32_t next()
    {
        const uint8_t* q = row + (size_t)x * ch;
        uint32_t v;
        if (ch == 4) {
            if (((uintptr_t)q & 3u) == 0) v = *reinterpret_cast<const uint32_t*>(q);
            else v = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
        } else {
            v = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | 0xFF000000u;
        }
        if (++x == w) { x = 0; row += pitch; }
        return v;
    }
};

// the pixel before tile t's first one ((0,0,0,255) before the image, qoi.d:334-338)
__device__ __forceinline__ uint32_t enc_prev(const EncImg& im, uint32_t p0)
{
    if (p0 == 0) return 0xFF000000u;
    EncReader r; r.seek(im, p0 - 1);
    return r.next();
}

__global__ __launch_bounds__(kLanes) void k_enc_summary(const EncImg* imgs, int n_img, uint32_t n_tiles, uint32_t* tab, TileMeta* meta)
{
    __shared__ uint32_t table[64 * kLanes];
    const int lane = threadIdx.x;
    const uint32_t g = blockIdx.x * kLanes + lane;
    if (g >= n_tiles) return;
    const EncImg im = imgs[find_unit<&EncImg::tile0>(imgs, n_img, g)];
    const uint32_t p0 = (g - im.tile0) * kTile, len = min((uint32_t)kTile, im.npx - p0);
    uint32_t prev = enc_prev(im, p0), trail = 0, allrep = 1;
    uint64_t mask = 0;
    EncReader r; r.seek(im, p0);
    for (uint32_t k = 0; k < len; ++k) {
        const uint32_t px = r.next();
        if (px == prev) { ++trail; continue; }
        const uint32_t h = enc_hash(px);
        table[h * kLanes + lane] = px;
        mask |= 1ull << h;
        trail = 0; allrep = 0; prev = px;
    }
    uint32_t* t = tab + (size_t)g * 64;
    for (int s = 0; s < 64; ++s) t[s] = (mask >> s & 1u) ? table[s * kLanes + lane] : 0u;
    meta[g] = TileMeta{ (uint32_t)mask, (uint32_t)(mask >> 32), allrep, trail };
}

// one wave per image, lane = hash slot: tab[tile] := the table entering the tile; run_in[tile] := the run counter entering it
__global__ __launch_bounds__(64) void k_enc_carry(const EncImg* imgs, uint32_t* tab, const TileMeta* meta, uint32_t* run_in)
{
    const EncImg im = imgs[blockIdx.x];
    const int lane = threadIdx.x;
    uint32_t cur = 0, run = 0;
    for (uint32_t t0 = 0; t0 < im.ntiles; t0 += kCarryAhead) {
        const uint32_t n = min((uint32_t)kCarryAhead, im.ntiles - t0);
        uint32_t v[kCarryAhead]; TileMeta m[kCarryAhead];
        #pragma unroll
        for (int j = 0; j < kCarryAhead; ++j)
            if ((uint32_t)j < n) { v[j] = tab[(size_t)(im.tile0 + t0 + j) * 64 + lane]; m[j] = meta[im.tile0 + t0 + j]; }
        #pragma unroll
        for (int j = 0; j < kCarryAhead; ++j) {
            if ((uint32_t)j >= n) break;
            const uint32_t g = im.tile0 + t0 + j;
            tab[(size_t)g * 64 + lane] = cur;
            if (lane == 0) run_in[g] = run;
            const uint32_t bit = lane < 32 ? m[j].mask_lo >> lane & 1u : m[j].mask_hi >> (lane - 32) & 1u;
            if (bit) cur = v[j];
            const uint32_t len = min((uint32_t)kTile, im.npx - (t0 + j) * kTile);
            run = m[j].allrep ? (run + len) % 62u : m[j].trail % 62u;          // the counter restarts at 62 (qoi.d:371-374)
        }
    }
}

// qoi.d:361-422 on one tile, from the carried-in state.  EMIT = 0: cnt[tile] = the tile's bytes; EMIT = 1: the bytes, at
// out + out_off + off[tile]
template <int EMIT>
__global__ __launch_bounds__(kLanes) void k_enc_walk(const EncImg* imgs, int n_img, uint32_t n_tiles, const uint32_t* tab, const uint32_t* run_in,
                                                      uint32_t* cnt, const uint32_t* off, uint8_t* out)
{
    __shared__ uint32_t table[64 * kLanes];
    const int lane = threadIdx.x;
    const uint32_t g = blockIdx.x * kLanes + lane;
    if (g >= n_tiles) return;
    const EncImg im = imgs[find_unit<&EncImg::tile0>(imgs, n_img, g)];
    const uint32_t p0 = (g - im.tile0) * kTile, len = min((uint32_t)kTile, im.npx - p0), last = im.npx - 1 - p0;
    const uint32_t* t = tab + (size_t)g * 64;
    for (int s = 0; s < 64; ++s) table[s * kLanes + lane] = t[s];
    uint32_t prev = enc_prev(im, p0), run = run_in[g], n = 0;
    // EMIT: bytes wait in `acc` and leave as dword stores once the write position is 4-aligned (a byte at a time until it is): a lane's
    // stores go to its own stretch of the stream, one per four bytes instead of one per byte
    uint8_t* o = EMIT ? out + im.out_off + off[g] : nullptr;
    uint64_t acc = 0; uint32_t na = 0, at = 0;
    auto put = [&](uint32_t b) {
        ++n;
        if (!EMIT) return;
        acc |= (uint64_t)b << (8 * na); ++na;
        if (((uintptr_t)(o + at) & 3u) != 0) { o[at++] = (uint8_t)acc; acc >>= 8; --na; }
        else if (na >= 4) { *reinterpret_cast<uint32_t*>(o + at) = (uint32_t)acc; at += 4; acc >>= 32; na -= 4; }
    };
    EncReader r; r.seek(im, p0);
    for (uint32_t k = 0; k < len; ++k) {
        const uint32_t px = r.next();
        if (px == prev) {
            ++run;
            if (run == 62 || k == last) { put(0xC0u | (run - 1)); run = 0; }
            continue;
        }
        if (run) { put(0xC0u | (run - 1)); run = 0; }
        const uint32_t h = enc_hash(px);
        uint32_t& slot = table[h * kLanes + lane];
        if (slot == px) {
            put(h);                                                            // QOI_OP_INDEX
        } else {
            slot = px;
            if ((px >> 24) == (prev >> 24)) {
                const int vr = (int8_t)(uint8_t)(px - prev), vg = (int8_t)(uint8_t)((px >> 8) - (prev >> 8)),
                          vb = (int8_t)(uint8_t)((px >> 16) - (prev >> 16));
                const int vg_r = (int8_t)(uint8_t)(vr - vg), vg_b = (int8_t)(uint8_t)(vb - vg);
                if (vr > -3 && vr < 2 && vg > -3 && vg < 2 && vb > -3 && vb < 2) {
                    put(0x40u | (uint32_t)(vr + 2) << 4 | (uint32_t)(vg + 2) << 2 | (uint32_t)(vb + 2));          // QOI_OP_DIFF
                } else if (vg_r > -9 && vg_r < 8 && vg > -33 && vg < 32 && vg_b > -9 && vg_b < 8) {
                    put(0x80u | (uint32_t)(vg + 32)); put((uint32_t)(vg_r + 8) << 4 | (uint32_t)(vg_b + 8));      // QOI_OP_LUMA
                } else {
                    put(0xFEu); put(px & 255u); put(px >> 8 & 255u); put(px >> 16 & 255u);                       // QOI_OP_RGB
                }
            } else {
                put(0xFFu); put(px & 255u); put(px >> 8 & 255u); put(px >> 16 & 255u); put(px >> 24);           // QOI_OP_RGBA
            }
        }
        prev = px;
    }
    if (EMIT) for (; na; --na) { o[at++] = (uint8_t)acc; acc >>= 8; }
    else cnt[g] = n;
}

// one workgroup per image: off[tile] = header + the bytes of the tiles before it; header, padding, stream length
constexpr int kScanThreads = 256;
__global__ __launch_bounds__(kScanThreads) void k_enc_scan(const EncImg* imgs, const uint32_t* cnt, uint32_t* off, int64_t* out_len, uint8_t* out)
{
    __shared__ uint32_t part[kScanThreads];
    const EncImg im = imgs[blockIdx.x];
    const int tid = threadIdx.x;
    const uint32_t per = (im.ntiles + kScanThreads - 1) / kScanThreads, b = min(im.ntiles, tid * per), e = min(im.ntiles, b + per);
    uint32_t s = 0;
    for (uint32_t t = b; t < e; ++t) s += cnt[im.tile0 + t];
    part[tid] = s;
    __syncthreads();
    for (int d = 1; d < kScanThreads; d <<= 1) {                               // inclusive Hillis-Steele scan of the parts
        const uint32_t add = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += add;
        __syncthreads();
    }
    uint32_t at = kHeader + part[tid] - s;
    for (uint32_t t = b; t < e; ++t) { off[im.tile0 + t] = at; at += cnt[im.tile0 + t]; }
    if (tid == 0) {
        const uint32_t body = part[kScanThreads - 1];
        uint8_t* o = out + im.out_off;
        const uint8_t hdr[kHeader] = { 'q', 'o', 'i', 'f', (uint8_t)(im.w >> 24), (uint8_t)(im.w >> 16), (uint8_t)(im.w >> 8), (uint8_t)im.w,
                                       (uint8_t)(im.h >> 24), (uint8_t)(im.h >> 16), (uint8_t)(im.h >> 8), (uint8_t)im.h,
                                       (uint8_t)im.ch, (uint8_t)im.colorspace };
        for (int k = 0; k < kHeader; ++k) o[k] = hdr[k];
        for (int k = 0; k < kPadding; ++k) o[kHeader + body + k] = k == kPadding - 1 ? 1 : 0;
        out_len[blockIdx.x] = (int64_t)kHeader + body + kPadding;
    }
}

// qoi.d:303-315: the worst-case stream length, 0 when qoi_encode refuses the desc
int64_t encode_bound(const gamut_hip_qoi_desc* d)
{
    if (!d || d->width == 0 || d->height == 0 || d->channels < 3 || d->channels > 4 || d->colorspace > 1 || d->height >= kPixelsMax / d->width)
        return 0;
    return (int64_t)d->width * d->height * (d->channels + 1) + kHeader + kPadding;
}

int encode_batch(const uint8_t* const* src, const int64_t* src_pitch, const gamut_hip_qoi_desc* descs, int count, const int64_t* out_offset,
                 uint8_t* out, int64_t* out_len, int* status_host, hipStream_t stream)
{
    std::vector<EncImg> imgs; std::vector<int> which;
    int first_bad = -1;
    uint64_t tiles = 0;
    for (int i = 0; i < count; ++i) {
        out_len[i] = 0;
        const bool ok = encode_bound(&descs[i]) > 0 && src[i] && out_offset[i] >= 0;
        if (status_host) status_host[i] = ok ? GAMUT_HIP_OK : GAMUT_HIP_ERR_INVALID_ARG;
        if (!ok) { if (first_bad < 0) first_bad = i; continue; }
        EncImg im{};
        im.src = src[i]; im.pitch = src_pitch[i]; im.out_off = out_offset[i];
        im.w = descs[i].width; im.h = descs[i].height; im.npx = im.w * im.h; im.ch = descs[i].channels; im.colorspace = descs[i].colorspace;
        im.tile0 = (uint32_t)tiles; im.ntiles = (im.npx + kTile - 1) / kTile;
        tiles += im.ntiles;
        if (tiles > 0x7FFFFFFFull / kLanes) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "qoi_encode: batch of more than %u tiles", 0x7FFFFFFFu / kLanes);
        imgs.push_back(im); which.push_back(i);
    }
    if (!imgs.empty()) {
        const int n = (int)imgs.size();
        const uint32_t T = (uint32_t)tiles;
        const size_t o_img = 0, o_tab = up256(n * sizeof(EncImg)), o_meta = o_tab + up256((size_t)T * 256), o_run = o_meta + up256((size_t)T * sizeof(TileMeta)),
                     o_cnt = o_run + up256((size_t)T * 4), o_off = o_cnt + up256((size_t)T * 4), o_len = o_off + up256((size_t)T * 4), total = o_len + up256((size_t)n * 8);
        static thread_local PerDevice<DeviceScratch> scratch_pd;
        static thread_local PerDevice<PinnedScratch> pinned_pd;
        uint8_t* d = (uint8_t*)scratch_pd.cur().get(total, stream);
        uint8_t* h = pinned_pd.cur().get(up256(n * sizeof(EncImg)) + (size_t)n * 8, stream);
        if (!d || !h) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "qoi_encode: scratch allocation of %zu bytes failed", total);
        memcpy(h, imgs.data(), n * sizeof(EncImg));
        GAMUT_HIP_CHECK(hipMemcpyAsync(d + o_img, h, n * sizeof(EncImg), hipMemcpyHostToDevice, stream));
        const EncImg* dimg = (const EncImg*)(d + o_img);
        uint32_t* tab = (uint32_t*)(d + o_tab); TileMeta* meta = (TileMeta*)(d + o_meta);
        uint32_t* run = (uint32_t*)(d + o_run); uint32_t* cnt = (uint32_t*)(d + o_cnt); uint32_t* off = (uint32_t*)(d + o_off);
        int64_t* len = (int64_t*)(d + o_len);
        const dim3 grid((T + kLanes - 1) / kLanes);
        hipLaunchKernelGGL(k_enc_summary, grid, dim3(kLanes), 0, stream, dimg, n, T, tab, meta);
        hipLaunchKernelGGL(k_enc_carry, dim3(n), dim3(64), 0, stream, dimg, tab, (const TileMeta*)meta, run);
        hipLaunchKernelGGL(k_enc_walk<0>, grid, dim3(kLanes), 0, stream, dimg, n, T, (const uint32_t*)tab, (const uint32_t*)run, cnt, (const uint32_t*)nullptr, (uint8_t*)nullptr);
        hipLaunchKernelGGL(k_enc_scan, dim3(n), dim3(kScanThreads), 0, stream, dimg, (const uint32_t*)cnt, off, len, out);
        hipLaunchKernelGGL(k_enc_walk<1>, grid, dim3(kLanes), 0, stream, dimg, n, T, (const uint32_t*)tab, (const uint32_t*)run, (uint32_t*)nullptr, (const uint32_t*)off, out);
        if (int rc = launch_status("qoi_encode")) return rc;
        int64_t* hlen = (int64_t*)(h + up256(n * sizeof(EncImg)));
        GAMUT_HIP_CHECK(hipMemcpyAsync(hlen, len, (size_t)n * 8, hipMemcpyDeviceToHost, stream));
        GAMUT_HIP_CHECK(hipStreamSynchronize(stream));
        for (int k = 0; k < n; ++k) out_len[which[(size_t)k]] = hlen[k];
    }
    if (first_bad >= 0) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "image %d: qoi_encode: invalid desc or source", first_bad);
    return GAMUT_HIP_OK;
}

} // namespace
} // namespace gamut

using namespace gamut;

extern "C" {

int64_t gamut_hip_qoi_encode_bound(const gamut_hip_qoi_desc* desc) { return encode_bound(desc); }

int gamut_hip_qoi_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const gamut_hip_qoi_desc* descs, int count,
                                      const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host, void* stream)
{
    clear_error();
    if (count < 0 || (count > 0 && (!src || !src_pitch || !descs || !out_offset || !out || !out_len)))
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "qoi_encode_batch_device: bad arguments");
    if (count == 0) return GAMUT_HIP_OK;
    if (!have_device()) return GAMUT_HIP_ERR_NO_DEVICE;
    try {
        return encode_batch(src, src_pitch, descs, count, out_offset, out, out_len, status_host, pick_stream(stream));
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "qoi_encode_batch_device: out of host memory");
    }
}

// drop-in for qoi_encode (qoi.d:295): the pixels go up through pinned staging, rows packed; malloc'd stream or NULL
void* gamut_hip_qoi_encode(const void* data, const gamut_hip_qoi_desc* desc, int pitch_bytes, int* out_len)
{
    clear_error();
    if (!data || !desc || !out_len || encode_bound(desc) == 0) { set_error(GAMUT_HIP_ERR_INVALID_ARG, "qoi_encode: invalid arguments"); return nullptr; }
    if (!have_device()) return nullptr;
    return encode_host_image("qoi_encode", HostRows{ data, pitch_bytes, (size_t)desc->width * desc->channels, (int)desc->height, 1, 0 },
                             (size_t)encode_bound(desc), out_len,
        [&](const uint8_t* src, int64_t pitch, int64_t, int64_t off, uint8_t* d, int64_t* len, hipStream_t st) {
            int status = 0;
            return encode_batch(&src, &pitch, desc, 1, &off, d, len, &status, st);
        });
}

} // extern "C"
