/*
 * gamut_hip.h -- C ABI of the MI355X (gfx950) batched image-decode /
 * pixel-convert path for Gamut (AuburnSounds/gamut).
 *
 * This header is the drop-in boundary: plain C, pointers and sizes only, no
 * C++/torch types.  A D program binds it with `extern(C) nothrow @nogc`
 * prototypes (INTEGRATION.md shows the binding file).  Each entry point names
 * the reference interface it replaces (paths relative to the reference repo,
 * source/gamut/...).
 *
 * Conventions (mirroring the reference):
 *   - no exceptions, no aborts: functions return an int status (0 = ok) or a
 *     NULL pointer; gamut_hip_last_error() gives a static/thread-local C string
 *   - PixelType ordinals are exactly types.d:32-59 (l8 = 0 ... rgbapf32 = 17,
 *     unknown = -1); pitches are signed bytes (negative = stored bottom-up)
 *   - "host" entry points take host pointers, are synchronous, and return
 *     malloc()-compatible memory where the reference does (free() it)
 *   - "device" entry points take HBM pointers, enqueue on the given hipStream_t
 *     (passed as void*, NULL = HIP's null stream) and do not synchronise;
 *     results stay resident in HBM
 *   - thread-safe: no mutable global state besides lazily created per-thread
 *     streams; concurrent calls on different images are safe
 */
#ifndef GAMUT_HIP_H
#define GAMUT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------- */
enum {
    GAMUT_HIP_OK              = 0,
    GAMUT_HIP_ERR_INVALID_ARG = 1,
    GAMUT_HIP_ERR_UNSUPPORTED = 2,   /* e.g. planar/compressed PixelType: scanline.d:82-85 */
    GAMUT_HIP_ERR_OUT_OF_MEMORY = 3,
    GAMUT_HIP_ERR_HIP         = 4,   /* a HIP runtime call failed; see last_error */
    GAMUT_HIP_ERR_DECODE      = 5,   /* corrupt / unsupported stream */
    GAMUT_HIP_ERR_NO_DEVICE   = 6
};

/* ---- PixelType (types.d:32-59) ------------------------------------------- */
enum {
    GAMUT_PIXEL_unknown = -1,
    GAMUT_PIXEL_l8 = 0, GAMUT_PIXEL_l16, GAMUT_PIXEL_lf32,
    GAMUT_PIXEL_la8, GAMUT_PIXEL_la16, GAMUT_PIXEL_laf32,
    GAMUT_PIXEL_lap8, GAMUT_PIXEL_lap16, GAMUT_PIXEL_lapf32,
    GAMUT_PIXEL_rgb8, GAMUT_PIXEL_rgb16, GAMUT_PIXEL_rgbf32,
    GAMUT_PIXEL_rgba8, GAMUT_PIXEL_rgba16, GAMUT_PIXEL_rgbaf32,
    GAMUT_PIXEL_rgbap8, GAMUT_PIXEL_rgbap16, GAMUT_PIXEL_rgbapf32,
    GAMUT_PIXEL_COUNT
};

/* JPEG sampling modes (jpegload.d:117-118, JPEG_SUBSAMPLING) */
enum { GAMUT_JPGD_GRAYSCALE = 0, GAMUT_JPGD_YH1V1, GAMUT_JPGD_YH2V1, GAMUT_JPGD_YH1V2, GAMUT_JPGD_YH2V2 };

/* ---- runtime ------------------------------------------------------------- */
const char* gamut_hip_version(void);
/* number of visible GPUs (0 if none / no driver) */
int  gamut_hip_device_count(void);
/* bind the calling thread to `device` (-1 = keep current). Returns status. */
int  gamut_hip_init(int device);
void gamut_hip_shutdown(void);
/* message for the last non-zero status on this thread ("" if none) */
const char* gamut_hip_last_error(void);

/* device memory / stream helpers so a non-HIP host (D, C) can drive the batched API */
void* gamut_hip_device_malloc(size_t bytes);
void  gamut_hip_device_free(void* p);
void* gamut_hip_host_malloc_pinned(size_t bytes);
void  gamut_hip_host_free_pinned(void* p);
int   gamut_hip_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream);
int   gamut_hip_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream);
void* gamut_hip_stream_create(void);
void  gamut_hip_stream_destroy(void* stream);
int   gamut_hip_stream_synchronize(void* stream);

/* ---- K8/K9: scanline conversion matrix ------------------------------------
 * replaces scanlinesConvert (scanline.d:70-121) / scanlinesCopy (:37-55).
 * Same argument meaning; the interType/interBuf scratch arguments disappear
 * (the intermediate lives in registers).  Returns GAMUT_HIP_OK where the
 * reference returns true. */
int gamut_hip_pixel_type_size(int type);                       /* types.d:62-86 */
int gamut_hip_scanlines_inter_type(int srcType, int dstType);  /* scanline.d:25-31 */

/* host pointers; synchronous (H2D, kernel, D2H inside) */
int gamut_hip_scanlines_convert(int srcType, const uint8_t* src, int srcPitch,
                                int dstType, uint8_t* dst, int dstPitch,
                                int width, int height);
int gamut_hip_scanlines_copy(int type, const uint8_t* src, int srcPitch,
                             uint8_t* dst, int dstPitch, int width, int height);

/* HBM pointers; layered like Image.convertTo's layer loop (image.d:1273-1311):
 * layer L's first scanline is src + L*srcLayerOffset.  Asynchronous. */
int gamut_hip_scanlines_convert_device(int srcType, const void* src, int64_t srcPitch, int64_t srcLayerOffset,
                                       int dstType, void* dst, int64_t dstPitch, int64_t dstLayerOffset,
                                       int width, int height, int layers, void* stream);

/* Image.flipHorizontal (image.d:1475-1509) / flipVerticalPhysical (:1926-1954) in place: pixel x <-> pixel W - 1 - x of every
 * row, or row y <-> row H - 1 - y, of every layer.  Device pointers + signed pitch + layer offset, asynchronous; the host variant
 * stages one image through the GPU (up, flip, down) like the other host drop-ins. */
int gamut_hip_flip_device(int type, void* data, int64_t pitch, int64_t layerOffset, int width, int height, int layers, int vertical, void* stream);
int gamut_hip_flip(int type, uint8_t* data, int pitch, int width, int height, int vertical);

/* ---- K1-K4: JPEG block reconstruction --------------------------------------
 * replaces transform_mcu / transform_mcu_expand (jpegload.d:2120-2255), the
 * *Convert row functions (:2528-2823) and the output packing of
 * decompress_jpeg_image_from_stream (:3753-3802).
 *
 * Input per image = what decode_next_row (:2405-2525) hands to transform_mcu:
 * de-quantised int16 coefficients in natural order, 64 per block, blocks in
 * MCU order (calc_mcu_block_order :3076-3088: Y.. Cb Cr), MCUs row-major,
 * mcus_per_row = ceil(width / mcu_w), mcus_per_col = ceil(height / mcu_h).
 * max_zag (optional, may be NULL) is m_mcu_block_max_zag per block (:2512);
 * NULL means "dense": identical results for every block whose pass-1 outputs
 * stay below 2^18 in magnitude, which holds for all 8-bit sample data
 * ("sparse IDCT paths").
 * Output: rows of width*out_comps bytes (out_comps 1, 3 or 4: l8 / rgb8 / rgba8,
 * :3761-3801), out_pitch bytes apart. */
typedef struct gamut_hip_jpeg_desc {
    const int16_t* coeffs;      /* HBM */
    const uint8_t* max_zag;     /* HBM or NULL */
    uint8_t*       out;         /* HBM */
    int64_t        out_pitch;   /* bytes */
    int32_t        width, height;
    int32_t        scan_type;   /* GAMUT_JPGD_* */
    int32_t        out_comps;   /* 1, 3, 4 */
} gamut_hip_jpeg_desc;

/* `count` independent images, arbitrary sizes. descs is a HOST array. Async. */
int gamut_hip_jpeg_reconstruct_device(const gamut_hip_jpeg_desc* descs, int count, void* stream);

/* uniform batch: image i uses coeffs + i*coeff_stride (int16 elements),
 * max_zag + i*zag_stride (bytes, ignored if max_zag NULL), out + i*out_stride
 * (bytes).  One launch for the whole batch.  Async. */
int gamut_hip_jpeg_reconstruct_batch_device(const int16_t* coeffs, int64_t coeff_stride,
                                            const uint8_t* max_zag, int64_t zag_stride,
                                            uint8_t* out, int64_t out_pitch, int64_t out_stride,
                                            int width, int height, int scan_type, int out_comps,
                                            int count, void* stream);

/* host-side feeder: entropy decode of one file into the dense form above --
 * baseline SOF0/SOF1 (jpegload.d:1160-1848 markers, :2405-2525 decode_next_row) and
 * progressive SOF2 (:3296-3664 scans into coefficient planes, :2259-2333 hand-over).
 * The frame's buffers are malloc'd; release with gamut_hip_jpeg_frame_free. */
typedef struct gamut_hip_jpeg_frame {
    int32_t  width, height, comps, scan_type;
    int32_t  mcus_per_row, mcus_per_col, blocks_per_mcu;
    int16_t* coeffs;            /* host */
    uint8_t* max_zag;           /* host */
    float    pixel_aspect_ratio, dpi_y;   /* what decompress_jpeg_image_from_stream hands out (jpegload.d:3804-3805): from the last JFIF (APP0) / EXIF (APP1) segment the
                                             decoder met -- in front of the frame, between scans or behind the last MCU row (find_eoi); JFIF without a unit: dpi_y -1;
                                             a file with neither: NaN (the D struct's float members are never assigned, :510-512), NOT the -1 of :3719's comment */
} gamut_hip_jpeg_frame;
int  gamut_hip_jpeg_decode_coeffs(const uint8_t* data, size_t len, gamut_hip_jpeg_frame* out);
void gamut_hip_jpeg_frame_free(gamut_hip_jpeg_frame* f);
/* header walk only (markers up to the first SOS): geometry and JFIF density; coeffs / max_zag stay NULL.  Lets a caller
 * size and lay out device buffers: an image needs mcus_per_row * mcus_per_col * blocks_per_mcu blocks of 64 int16. */
int  gamut_hip_jpeg_read_header(const uint8_t* data, size_t len, gamut_hip_jpeg_frame* out);
/* what the device entropy decoder would be given for this file: the geometry, the number of independently
 * decodable segments (restart intervals, or 1; for a progressive file: summed over its scans) and the size of the
 * unstuffed entropy-coded data with its padding.
 * Host only; the same preparation code gamut_hip_jpeg_entropy_decode_device runs per file. */
int  gamut_hip_jpeg_scan_layout(const uint8_t* data, size_t len, gamut_hip_jpeg_frame* info, int32_t* segments, uint64_t* entropy_bytes);
/* Entropy decode ON THE DEVICE of `count` baseline files given in host memory: the compressed
 * scans are uploaded (unstuffed on host threads straight into pinned memory, DMA on a private copy stream overlapped with
 * the decode of the files already there) and a workgroup of self-synchronising lanes per scan -- a lane per restart
 * interval where the file has short ones -- writes the
 * dense de-quantised coefficient form (what decode_next_row, jpegload.d:2405-2525, leaves per MCU row) into
 * coeffs[coeff_offset[i] ..] (int16 elements) and max_zag[zag_offset[i] ..] (device pointers, caller-sized from
 * gamut_hip_jpeg_read_header).  Progressive (SOF2) files of the batch (jpegload.d:3296-3664) go to the same buffers: their
 * scans are decoded level by level on the device -- every scan of a level of every file in one launch; AC refinement
 * blocks a wave each -- then de-quantised in place (gamut_amd/csrc/jpeg_prog.hpp); fewer than twelve such files per host
 * thread are decoded by the host feeder and uploaded instead (GAMUT_HIP_JPEG_PROGRESSIVE=host / device forces either).
 * info[i] receives the geometry and the density (host), status_host[i] (may be NULL) the per-file verdict, and status_dev[i]
 * (device, may be NULL) is non-zero only for a file the call refuses.  What a kernel cannot vouch for -- a bit pattern no code word
 * begins, a segment that runs out, a wrong or missing RSTn, octets between an interval's last bit and its marker; the reference has a
 * result for most of these (jpgd decodes symbol 0 and carries on, huff_decode :746-813) -- is decoded again by the host feeder
 * (gamut_hip_jpeg_decode_coeffs) behind the device pass and uploaded, so a damaged file costs a host decode, an intact one nothing; the
 * markers behind the scan (find_eoi :2826-2848) are walked on the host from where the device saw the scan end.
 * Returns when the decode has finished on `stream`;
 * the status of the lowest-numbered failing file, GAMUT_HIP_OK if none. */
int  gamut_hip_jpeg_entropy_decode_device(const uint8_t* const* data, const size_t* len, int count,
                                          const int64_t* coeff_offset, const int64_t* zag_offset,
                                          int16_t* coeffs, uint8_t* max_zag, uint32_t* status_dev,
                                          gamut_hip_jpeg_frame* info, int* status_host, void* stream);
/* Files -> pixels: `count` JPEG files in host memory (baseline and progressive, any sampling mode) -> rows of
 * width * req_comps bytes (req_comps = 1 / 3 / 4: l8 / rgb8 / rgba8, as decompress_jpeg_image_from_memory converts) at
 * out + out_offset[i] (device).  The JPEG member of the trio of file-level batch calls (with gamut_hip_png_decode_batch_device and
 * gamut_hip_qoi_decode_batch_device: BASELINE.json config 5 end to end).  It is gamut_hip_jpeg_entropy_decode_device followed by
 * the reconstruction kernels, except that the library owns the coefficient buffers (per-thread device scratch, sized from the
 * headers) and that a group's reconstruction is queued right behind ITS entropy decode, beside the decode of the next group and
 * the upload of the one after.  info[i] receives the geometry, status_host[i] / status_dev[i]
 * (both may be NULL) as above.  Returns when the pixels are in place; the status of the lowest-numbered failing file. */
int  gamut_hip_jpeg_decode_batch_device(const uint8_t* const* data, const size_t* len, int count, int req_comps,
                                        const int64_t* out_offset, uint8_t* out, gamut_hip_jpeg_frame* info, int* status_host,
                                        uint32_t* status_dev, void* stream);
/* the same for `count` independent files on up to `threads` host threads (<= 0: one per hardware thread).  The reference
 * decodes one image at a time (the serial Huffman stage is what bounds a batch once the GPU stages
 * run at HBM speed).  status[i] (may be NULL) receives image i's status and out[i] its frame (zeroed on failure);
 * returns GAMUT_HIP_OK when every image decoded, otherwise the status of the lowest-numbered failing image. */
int  gamut_hip_jpeg_decode_coeffs_batch(const uint8_t* const* data, const size_t* len, int count,
                                        gamut_hip_jpeg_frame* out, int* status, int threads);

/* drop-in for decompress_jpeg_image_from_stream (jpegload.d:3720-3723) on a
 * memory buffer: host entropy decode, GPU reconstruction, malloc'd
 * width*req_comps*height result (NULL on failure).  req_comps -1/1/3/4. */
uint8_t* gamut_hip_decompress_jpeg_image_from_memory(const uint8_t* data, size_t len,
        int* width, int* height, int* actual_comps,
        float* pixelAspectRatio, float* dotsPerInchY, int req_comps);

/* the same with the reference's own argument list (jpegload.d:3720-3723): the input arrives through a JpegStreamReadFunc
 * (jpegload.d:61-70): `int function(void* pBuf, int max_bytes_to_read, bool* pEOF_flag, void* userData)`, -1 = error, called
 * until it raises *pEOF_flag.  D's bool is one byte: unsigned char here.  The stream is pulled in jpgd's own 8 KiB pieces
 * (prep_in_buffer, jpegload.d:1971-2003) and no further call is made once the image's EOI marker has arrived -- an image
 * embedded in a longer stream is over-read by less than one piece, as by the reference -- then decoded as above. */
typedef int (*gamut_hip_jpeg_stream_read_func)(void* pBuf, int max_bytes_to_read, unsigned char* pEOF_flag, void* userData);
uint8_t* gamut_hip_decompress_jpeg_image_from_stream(gamut_hip_jpeg_stream_read_func rfn, void* userData,
        int* width, int* height, int* actual_comps,
        float* pixelAspectRatio, float* dotsPerInchY, int req_comps);

/* ---- K5-K7: PNG de-filter / expand -----------------------------------------
 * replaces stbi__create_png_image_raw (stbdec.d:1406-1635).  raw = inflated
 * stream of one non-interlaced image (or one Adam7 pass): per row one filter
 * byte + ceil(img_n*x*depth/8) bytes.  out = x*y*out_n*(depth==16?2:1) bytes,
 * tightly packed, out_n == img_n or img_n+1 (alpha = 255 inserted), 1/2/4-bit
 * samples expanded (grey scaled when color==0), 16-bit samples native-endian. */
typedef struct gamut_hip_png_desc {
    const uint8_t* raw;         /* HBM */
    uint8_t*       out;         /* HBM */
    uint32_t       raw_len;
    uint32_t       x, y;
    int32_t        img_n, out_n, depth, color;
} gamut_hip_png_desc;
/* status (HBM, may be NULL): one uint32 per image, bit 0 is set when a row carries an invalid
 * filter type (> 4, "Corrupt PNG" stbdec.d:1438); zero it before the call. */
int gamut_hip_png_defilter_device(const gamut_hip_png_desc* descs, int count, uint32_t* status, void* stream);

/* uniform batch: image i uses raw + i*raw_stride, out + i*out_stride (bytes). */
int gamut_hip_png_defilter_batch_device(const uint8_t* raw, int64_t raw_stride, uint32_t raw_len,
                                        uint8_t* out, int64_t out_stride,
                                        uint32_t x, uint32_t y, int img_n, int out_n, int depth, int color,
                                        int count, uint32_t* status, void* stream);

/* drop-ins for stbi_load_from_callbacks / stbi_load_16_from_callbacks
 * (stbdec.d:713-735) on a memory buffer: host chunk parse + inflate, GPU
 * de-filter/expand/post passes, malloc'd result (NULL on failure). */
uint8_t*  gamut_hip_stbi_load_from_memory(const uint8_t* data, size_t len, int* x, int* y, int* comp, int req_comp,
                                          float* ppmX, float* ppmY, float* pixelRatio);
uint16_t* gamut_hip_stbi_load_16_from_memory(const uint8_t* data, size_t len, int* x, int* y, int* comp, int req_comp,
                                             float* ppmX, float* ppmY, float* pixelRatio);
/* stbi__png_is16 (stbdec.d:2091-2109) */
int gamut_hip_png_is16(const uint8_t* data, size_t len);
/* the same three with the reference's own argument lists: stbi_io_callbacks (stbdec.d:408-419) + the user pointer, then
 * exactly the parameters of stbi_load_from_callbacks / stbi_load_16_from_callbacks (stbdec.d:713-735).  The stream is walked
 * chunk by chunk as stbi__parse_png_file does (stbdec.d:1777-2023): `read` for chunk headers and the chunks the parser looks
 * at (a read of 0 bytes ends the data, as in stbi__refill_buffer :780-795), `skip` for every other ancillary chunk
 * (stbi__skip :822-842; NULL = read and drop), `eof` for the file without IEND (:2008-2012; NULL = "not yet").  The walk stops
 * behind IEND's CRC and leaves the stream there (stb's 128-byte buffer leaves it up to 127 bytes further): a second image may
 * follow in the same stream.  is16 reads up to IHDR only; the caller rewinds its stream before loading, as
 * plugins/png.d:50-62 does. */
typedef struct gamut_hip_stbi_io_callbacks {
    int  (*read)(void* user, char* data, int size);
    void (*skip)(void* user, int n);
    int  (*eof)(void* user);
} gamut_hip_stbi_io_callbacks;
uint8_t*  gamut_hip_stbi_load_from_callbacks(const gamut_hip_stbi_io_callbacks* clbk, void* user, int* x, int* y, int* comp, int req_comp,
                                             float* ppmX, float* ppmY, float* pixelRatio);
uint16_t* gamut_hip_stbi_load_16_from_callbacks(const gamut_hip_stbi_io_callbacks* clbk, void* user, int* x, int* y, int* comp, int req_comp,
                                                float* ppmX, float* ppmY, float* pixelRatio);
int gamut_hip_stbi_png_is16_from_callbacks(const gamut_hip_stbi_io_callbacks* clbk, void* user);

/* ---- inflate on the GPU -------------------------------------------------------------------
 * replaces, for batches, stbi_zlib_decode_malloc_guesssize_headerflag (stbdec.d:1267-1321 -> miniz).  Stream i is the raw
 * DEFLATE data src[0 .. src_len) in HBM (a zlib stream without its 2-byte header, which the host checks as stbdec.d does;
 * the adler32 trailer is not read, as with the reference's trusted_input); its bytes go to dst[0 .. dst_cap) in HBM -- output
 * beyond dst_cap is dropped (the de-filter needs (bytes per line + 1) * height, no more), but the stream is still decoded to its
 * end: damage anywhere makes it a corrupt stream, as for the reference, which inflates all of it.
 * out_len_dev[i] = bytes written, status_dev[i] = 0 or the reason the stream is corrupt (GAMUT_HIP_INFLATE_E_*); both are
 * device arrays, the call is asynchronous on `stream`.  One 1024-thread workgroup per stream: speculative parallel Huffman
 * decode into a token list, then parallel match resolution tile by tile (gamut_amd/csrc/inflate.hip); the library keeps 256 KiB
 * of HBM scratch per RESIDENT workgroup (two per compute unit: 128 MiB on MI355X however many streams a batch has) plus small per-stream
 * tables, per (thread, device, stream).  descs is a host array.  One deviation from zlib, as a
 * bound on the work a hostile stream can demand: a stream with more than 4096 + src_len / 8 blocks (no encoder comes near:
 * that is a block per 8 compressed bytes) is reported as GAMUT_HIP_INFLATE_E_INPUT. */
typedef struct gamut_hip_inflate_desc { const uint8_t* src; uint8_t* dst; uint32_t src_len, dst_cap; } gamut_hip_inflate_desc;
enum { GAMUT_HIP_INFLATE_E_BLOCK_TYPE = 1, GAMUT_HIP_INFLATE_E_STORED = 2, GAMUT_HIP_INFLATE_E_LENGTHS = 3, GAMUT_HIP_INFLATE_E_CODE = 4,
       GAMUT_HIP_INFLATE_E_DISTANCE = 5, GAMUT_HIP_INFLATE_E_INPUT = 6 };
int gamut_hip_inflate_batch_device(const gamut_hip_inflate_desc* descs, int count, uint32_t* out_len_dev, uint32_t* status_dev, void* stream);
/* The same in several launches, each allowed `slice_bytes` more of every stream than the one before: a stream stops in front of what it
 * cannot finish within the bytes it may read and goes on from its saved state (position, code lengths of the block it stands in; the
 * window comes back from its output).  This is how gamut_hip_png_decode_batch_device inflates while the files are still on their way
 * over PCIe; here all bytes are in HBM already -- same results as the call above, for tests and measurements (this one returns when the
 * last launch has finished). */
int gamut_hip_inflate_batch_device_sliced(const gamut_hip_inflate_desc* descs, int count, uint32_t* out_len_dev, uint32_t* status_dev, uint32_t slice_bytes, void* stream);

/* ---- PNG files in batches ----------------------------------------------------------------------------------- */
typedef struct gamut_hip_png_info {
    uint32_t width, height;
    int32_t  channels_in_file;      /* what stbi reports as *comp: 1..4 (palette images: 3 or 4) */
    int32_t  channels;              /* of the decoded pixels: req_comp, or channels_in_file when req_comp == 0 */
    int32_t  bits;                  /* of the decoded samples: 8 or 16 */
    float    pixels_per_meter_x, pixels_per_meter_y, pixel_aspect_ratio;   /* pHYs, -1 when absent */
} gamut_hip_png_info;
/* IHDR only (host): width, height, bit depth class and the channel count implied by the colour type */
int gamut_hip_png_read_header(const uint8_t* data, size_t len, gamut_hip_png_info* info);
/* `count` PNG files in host memory -> pixels at out + out_offset[i] (device): chunk walk + inflate on up to `threads` host
 * threads (<= 0: one per hardware thread; the inflate is what bounds a PNG pipeline), the inflated streams going to the
 * device as they finish; then the rest of stbi__do_png on the GPU -- files that only need de-filter + expand are
 * de-filtered together, one launch per geometry (one workgroup per image), the others stage by stage per file.  Batches of
 * more files than host threads inflate on the GPU instead (gamut_hip_inflate_batch_device: the threads then only walk
 * the chunks and gather the IDAT bytes for one upload); the environment variable GAMUT_HIP_PNG_INFLATE=host / device forces
 * either.  req_comp as in stbi_load (0 = as in the file), bits = 8 / 16 as stbi_load / stbi_load_16 convert, 0 = as
 * in the file.  info[i] / status_host[i] (may be NULL) per file; returns the status of the lowest-numbered failing file. */
int gamut_hip_png_decode_batch_device(const uint8_t* const* data, const size_t* len, int count, int req_comp, int bits,
                                      const int64_t* out_offset, uint8_t* out, gamut_hip_png_info* info, int* status_host,
                                      int threads, void* stream);

/* ---- QOI (codecs/qoi.d) -- SURVEY.md 8f row N4 ---------------------------------------------------------------- */
typedef struct gamut_hip_qoi_desc { uint32_t width, height; uint8_t channels, colorspace; } gamut_hip_qoi_desc;   /* qoi_desc, decode fields */
/* drop-in for qoi_decode (qoi.d:448-550): channels = 0 (as in the file), 3 or 4; malloc'd width*height*channels bytes, or
 * NULL with the same header checks (:458-480).  Decoded on the GPU (one lane per stream). */
void* gamut_hip_qoi_decode(const void* data, int size, gamut_hip_qoi_desc* desc, int channels);
/* header only (host) */
int   gamut_hip_qoi_read_header(const void* data, int size, gamut_hip_qoi_desc* desc);
/* batch: `count` streams in host memory -> pixels at out + out_offset[i] (device), one lane per image.  descs[i] (host)
 * receives the headers, status_host[i] (may be NULL) the per-file header status.  Returns when the decode has finished. */
int   gamut_hip_qoi_decode_batch_device(const uint8_t* const* data, const int* size, int count, int channels,
                                        const int64_t* out_offset, uint8_t* out, gamut_hip_qoi_desc* descs, int* status_host, void* stream);
/* the same decode for files that are already resident in HBM (a device-side file cache; bench.py's mixed workload): file i
 * is blob[begin[i] .. begin[i] + size[i]) and must be followed by GAMUT_HIP_QOI_SLACK readable bytes inside the blob (the
 * lanes read whole 64-byte blocks); begin / size / descs (from gamut_hip_qoi_read_header) / out_offset are host arrays,
 * read before the call returns.  Asynchronous on `stream`, like the other device entry points. */
#define GAMUT_HIP_QOI_SLACK 160
int   gamut_hip_qoi_decode_resident_device(const uint8_t* blob, int64_t blob_len, const int64_t* begin, const int* size,
                                           const gamut_hip_qoi_desc* descs, int count, int channels, const int64_t* out_offset,
                                           uint8_t* out, void* stream);
/* QOI encode (qoi_encode, qoi.d:295-436), byte for byte.  The worst-case stream length (:313-315), or 0 when qoi_encode would refuse
 * the desc (:303-311: zero width or height, channels other than 3 / 4, colorspace > 1, height >= 400000000 / width). */
int64_t gamut_hip_qoi_encode_bound(const gamut_hip_qoi_desc* desc);
/* drop-in for qoi_encode: the reference desc's pitchBytes passed beside it (rows of `data` are pitch_bytes apart, negative allowed);
 * malloc'd stream of *out_len bytes, or NULL (bad arguments, no device: see last_error).  Encoded on the GPU. */
void*   gamut_hip_qoi_encode(const void* data, const gamut_hip_qoi_desc* desc, int pitch_bytes, int* out_len);
/* batch: image i is read from DEVICE memory at src[i] with rows src_pitch[i] apart (negative allowed, any alignment) and encoded to
 * out + out_offset[i] (device), which must have gamut_hip_qoi_encode_bound(&descs[i]) bytes; nothing outside
 * [out_offset[i], out_offset[i] + out_len[i]) is written.  out_len[i] / status_host[i] (host arrays; status_host may be NULL) receive
 * the stream length and per-image status: an image the reference would refuse (or a NULL src[i], a negative out_offset[i]) gets
 * GAMUT_HIP_ERR_INVALID_ARG and out_len 0, the others are still encoded, and the call returns the status of the lowest-numbered
 * refused image.  Returns when the encode has finished. */
int     gamut_hip_qoi_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const gamut_hip_qoi_desc* descs,
                                          int count, const int64_t* out_offset, uint8_t* out, int64_t* out_len,
                                          int* status_host, void* stream);

/* JPEG encode (stbi_write_jpg_core, stb_image_write.d:632-880), byte for byte: baseline, three components (comp 1 and 2 are grey,
 * the alpha of comp 2 and 4 is ignored), 4:2:0 when quality <= 90 (0 means 90) and 4:4:4 above, standard Annex K tables.
 * Refused: NULL data, width or height below 1, comp outside 1..4, and -- unlike the reference, which writes a truncated SOF0 --
 * width or height above 65535.
 * The worst-case stream length, or 0 when refused: 607 + 2 * ceil((blocks * 1660 + 7) / 8) + 2 bytes (1660 bits per 8x8 block at
 * most, every data byte possibly stuffed). */
int64_t gamut_hip_jpeg_encode_bound(int width, int height, int comp, int quality);
/* host pixels (rows `pitch` bytes apart, negative allowed) -> malloc'd stream of *out_len bytes, or NULL (see last_error).  Encoded
 * on the GPU through pinned staging. */
void*   gamut_hip_jpeg_encode(const void* data, int width, int height, int comp, int pitch, int quality, int* out_len);
/* drop-in for stbi_write_jpg_to_func: returns 1, or 0 on refusal without calling func.  The bytes handed to func, concatenated,
 * are the reference's; they come in one call rather than the reference's many small ones. */
typedef void (*gamut_hip_jpeg_write_func)(void* context, const void* data, int size);
int     gamut_hip_jpeg_write_to_func(gamut_hip_jpeg_write_func func, void* context, int x, int y, int comp, const void* data, int pitch,
                                     int quality);
/* batch: image i is read from DEVICE memory at src[i] (rows src_pitch[i] apart, negative allowed, any alignment), width[i] x
 * height[i], comp[i], quality[i] (quality may be NULL: 90 for every image), and encoded to out + out_offset[i] (device), which
 * must have gamut_hip_jpeg_encode_bound(...) bytes; nothing outside [out_offset[i], out_offset[i] + out_len[i]) is written.
 * out_len[i] / status_host[i] (host arrays; status_host may be NULL) receive the stream length and per-image status: a refused
 * image (or a NULL src[i], a negative out_offset[i]) gets GAMUT_HIP_ERR_INVALID_ARG and out_len 0, the others are still encoded,
 * and the call returns the status of the lowest-numbered refused image.  Returns when the encode has finished. */
int     gamut_hip_jpeg_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const int32_t* width,
                                           const int32_t* height, const int32_t* comp, const int32_t* quality, int count,
                                           const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host,
                                           void* stream);

/* PNG encode (stbi_write_png_to_mem, stb_image_write.d:254-451).  Container and filter stream are the reference's byte for byte:
 * inflate(IDAT payload) is the `filt` buffer it hands to its compressor (per-row filter choice included) and every byte outside
 * the IDAT payload is what it writes around a payload of that length.  The DEFLATE stream is this library's own (the reference's
 * miniz stream is not reproduced): a valid, deterministic zlib stream built on the GPU from independent blocks of 8192 filtered
 * bytes, each the smallest of stored / fixed / dynamic Huffman, matches of 3..258 at the distances filtered PNG data repeats at.
 * comp 1..4 (l, la, rgb, rgba), is16bit: samples are native 16-bit and written big-endian.  force_filter 0..4 forces a filter,
 * anything else selects per row as the reference does.  compression_level 0 writes stored blocks only; 1..10 all stand for the one
 * effort of the GPU compressor; no level produces a larger file than level 0.
 * Refused: NULL pixels, width or height below 1, comp outside 1..4, level outside 0..10, and any image whose filtered stream
 * (width * comp * (is16bit ? 2 : 1) + 1) * height does not fit a positive int (the reference's int arithmetic would wrap).
 * The worst-case file length, or 0 when refused, with L the filtered length above: 57 + 6 + L + 5 * ceil(L / 8192) -- the container,
 * the zlib header and Adler-32, and L bytes in stored blocks of 8192. */
int64_t gamut_hip_png_encode_bound(int width, int height, int comp, int is16bit);
/* drop-in for stbi_write_png_to_mem (same argument list): host pixels (rows stride_bytes apart, negative allowed) through pinned
 * staging -> malloc'd file of *out_len bytes, or NULL on refusal (see last_error). */
void*   gamut_hip_png_write_to_mem(const void* pixels, int stride_bytes, int x, int y, int n, int* out_len, int is16bit,
                                   int force_filter, int compression_level);
/* batch: image i is read from DEVICE memory at src[i] (rows src_pitch[i] apart, negative allowed, any alignment) and encoded to
 * out + out_offset[i] (device), which must have gamut_hip_png_encode_bound(...) bytes; nothing outside
 * [out_offset[i], out_offset[i] + out_len[i]) is written.  force_filter may be NULL (-1: select for every image), level may be
 * NULL (5).  out_len[i] / status_host[i] (host arrays; status_host may be NULL) receive the file length and per-image status: a
 * refused image (or a NULL src[i], a negative out_offset[i]) gets GAMUT_HIP_ERR_INVALID_ARG and out_len 0, the others are still
 * encoded, and the call returns the status of the lowest-numbered refused image.  Returns when the encode has finished. */
int     gamut_hip_png_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const int32_t* width,
                                          const int32_t* height, const int32_t* comp, const int32_t* is16bit,
                                          const int32_t* force_filter, const int32_t* level, int count, const int64_t* out_offset,
                                          uint8_t* out, int64_t* out_len, int* status_host, void* stream);

/* ---- BMP (stbi__bmp_load, codecs/stbdec.d:2112-2512; write_bmp, codecs/bmpenc.d; plugins/bmp.d) ---------------------------------
 * Decode: every pixel what stbi__bmp_load gives, bit for bit: 1 / 4 / 8-bit palette, 16 / 32-bit with masks, 24-bit and plain 32-bit,
 * header sizes 12 / 40 / 56 / 108 / 124, bottom-up and top-down, no RLE (the reference refuses it); the all-alpha-zero rule of 32-bit
 * BI_RGB files (:2137, :2439-2443) included.  Bytes past the end of a file read as zero, as the reference's reader hands them out.
 * Deliberate deviations: a palette index >= the palette size gives (0, 0, 0) (the reference reads uninitialised memory); a negative
 * palette size and a width or height of 0 are refused.
 * (Declared typedef-first: the layout of this struct is pinned by tests/c/bmp_abi_layout.c and tests/test_bmp_cpu.py.) */
typedef struct gamut_hip_bmp_info gamut_hip_bmp_info;
struct gamut_hip_bmp_info {
    int32_t  width, height;         /* height as a positive number */
    int32_t  bpp, header_size, compression;
    int32_t  channels_in_file;      /* what stbi reports as *comp: 3 or 4 */
    int32_t  top_down;              /* 1: the file's first row is the top one (negative biHeight) */
    int32_t  pixel_offset;          /* where the reference starts to read pixels (bmp_host.hip) */
    int32_t  palette_size;          /* entries, 0 for 16 / 24 / 32 bits */
    uint32_t mask_r, mask_g, mask_b, mask_a;
    float    pixels_per_meter_x, pixels_per_meter_y, pixel_aspect_ratio;   /* -1 when unknown (values <= 1 count as unknown) */
};
/* the header alone (host, no GPU needed): the reference's verdict on the file, GAMUT_HIP_ERR_DECODE when it would refuse it */
int gamut_hip_bmp_read_header(const uint8_t* data, size_t len, gamut_hip_bmp_info* info);
/* `count` BMP files in host memory -> tight rows of width * comps bytes at out + out_offset[i] (device); req_comp as in stbi_load:
 * 0 (as in the file), 1, 2, 3 or 4.  One launch for the whole batch, whatever the files' geometries and depths.  info[i] /
 * status_host[i] (either may be NULL) per file; a refused file gets its status and does not disturb the others; returns the status
 * of the lowest-numbered refused file.  Nothing outside an image's width * height * comps bytes is written.  Returns when the
 * pixels are in place. */
int gamut_hip_bmp_decode_batch_device(const uint8_t* const* data, const size_t* len, int count, int req_comp,
                                      const int64_t* out_offset, uint8_t* out, gamut_hip_bmp_info* info, int* status_host, void* stream);
/* measurements: with the environment variable GAMUT_HIP_BMP_TIMING=1 the decode call brackets its kernels (not the upload) with events;
 * this returns the GPU milliseconds of the calling thread's last decode call, -1 when timing is off or nothing was decoded */
float gamut_hip_bmp_last_decode_kernel_ms(void);
/* Encode: byte for byte write_bmp (bmpenc.d:25-114) -- a BITMAPV4 header of 122 bytes, rows bottom-up, B and R swapped; comp 3
 * (24 bits, BI_RGB) or 4 (32 bits, BI_BITFIELDS with the four masks), 1 <= width, height <= 32767 (plugins/bmp.d:174-189).
 * Deliberate deviation: the 0..3 pad bytes of a 24-bit row, which the reference writes from an uninitialised buffer, are zero.
 * The file length 122 + height * ((width * comp + 3) & ~3), or 0 when saveBMP / write_bmp would refuse the shape. */
int64_t gamut_hip_bmp_encode_bound(int width, int height, int comp);
/* batch: image i is read from DEVICE memory at src[i] (rows src_pitch[i] apart, negative allowed, any alignment) and written to
 * out + out_offset[i] (device, any alignment), which must have gamut_hip_bmp_encode_bound(...) bytes; nothing outside
 * [out_offset[i], out_offset[i] + out_len[i]) is written.  ppm_x / ppm_y: biXPelsPerMeter / biYPelsPerMeter per image, either
 * may be NULL (0).  out_len[i] / status_host[i] (host arrays; status_host may be NULL): a refused image (or a NULL src[i], a
 * negative out_offset[i]) gets GAMUT_HIP_ERR_INVALID_ARG and out_len 0, the others are still encoded, and the call returns the
 * status of the lowest-numbered refused image.  Returns when the encode has finished. */
int     gamut_hip_bmp_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const int32_t* width,
                                          const int32_t* height, const int32_t* comp, const int32_t* ppm_x, const int32_t* ppm_y,
                                          int count, const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host,
                                          void* stream);
/* host pixels (rows `pitch` bytes apart, negative allowed) through pinned staging -> malloc'd file of *out_len bytes, or NULL on
 * refusal (see last_error) */
void*   gamut_hip_bmp_write_to_mem(const void* data, int pitch, int w, int h, int comp, int ppm_x, int ppm_y, int* out_len);

/* ---- GIF (GIFDecoder, codecs/gif.d; loadGIF, plugins/gif.d:57-103) --------------------------------------------------------------
 * Decode: every frame of the file, composited as the reference composites it (its disposal rules, its persistent GCE state --
 * also from the counting pass of `open` into the decoding pass --, its pixel stepping for interlaced, overhanging and zero-sized
 * frames, its LZW verdicts), as `layers` tight rgba8 images of width x height.
 * Deliberate deviations (in each the reference reads or writes memory it does not own): both palette buffers start zeroed, so an
 * index past every colour table ever read gives an undrawn pixel; a frame with neither a local nor a global colour table is refused;
 * a frame with frameX + max(frameW, 1) > width is refused (one overhanging the BOTTOM is not: its rows are dropped as in the
 * reference); a screen of more than 2^29 - 1 pixels is refused.
 * (Declared typedef-first: the layout of this struct is pinned by tests/c/gif_abi_layout.c and tests/test_gif_cpu.py.) */
typedef struct gamut_hip_gif_info gamut_hip_gif_info;
struct gamut_hip_gif_info {
    int32_t width, height;          /* the logical screen */
    int32_t layers;                 /* frames in the file; 0 is a valid file */
    int32_t is_gif89;
    float   pixel_aspect_ratio;     /* (byte + 15) / 64, -1 when the byte is 0 */
    float   fps;                    /* layers * 1000 / sum of the frame durations in ms (100 for a delay of 0 or 1, else delay * 10); 10 when the sum is 0 */
};
/* host only, no GPU needed: the whole verdict of GIFDecoder.open -- the container and every LZW code of every frame -- with the
 * deviations above; GAMUT_HIP_ERR_DECODE where the file is refused (info is then zeroed, pixel_aspect_ratio -1) */
int gamut_hip_gif_read_header(const uint8_t* data, size_t len, gamut_hip_gif_info* info);
/* `count` GIF files in host memory; layer l of file i goes, as tight rgba8 rows, to out + out_offset[i] + l * width * height * 4
 * (device).  out_capacity[i]: the bytes file i may use; a file whose layers * width * height * 4 exceed it gets
 * GAMUT_HIP_ERR_INVALID_ARG (info[i] then tells what it needs; the test is made on what the container claims, before the raster is
 * looked at).  One LZW launch (a wave per frame) and one compositing launch for
 * the whole batch.  info[i] / status_host[i] (either may be NULL) per file; a refused file gets its status, leaves its slot
 * untouched and does not disturb the others; returns the status of the lowest-numbered refused file.  The raster verdict comes
 * from the LZW kernel's status words, not from the host's code walk.  Nothing outside a file's layers * width * height * 4 bytes is
 * written.  The files go up through pinned staging; returns when the pixels are in place. */
int gamut_hip_gif_decode_batch_device(const uint8_t* const* data, const size_t* len, int count, const int64_t* out_offset,
                                      const int64_t* out_capacity, uint8_t* out, gamut_hip_gif_info* info, int* status_host, void* stream);
/* measurements: with the environment variable GAMUT_HIP_GIF_TIMING=1 the decode call brackets its kernels (not the upload) with events;
 * this returns the GPU milliseconds of the calling thread's last decode call (both kernels), -1 when timing is off or nothing was
 * decoded.  gamut_hip_gif_last_kernel_ms is the same figure split in two, which = 0: the LZW kernel, 1: the compositing kernel.  It
 * exists because the two kernels are bound differently (a latency chain per frame / the layers' stores) and tools/gif_bench.py
 * records them apart; a measurement aid like the entry above, not part of the decode interface. */
float gamut_hip_gif_last_decode_kernel_ms(void);
float gamut_hip_gif_last_kernel_ms(int which);
/* Encode: byte for byte what saveGIF (plugins/gif.d:105-147) gets from msf_gif (codecs/msf_gif.d: begin, one msf_gif_frame per layer,
 * end) for a stack of rgba8 frames: the 32-byte header with the NETSCAPE2.0 loop block, per frame a GCE + image descriptor, a local
 * colour table of 1 << tableBits entries and the LZW stream in 255-byte sub-blocks, then 0x3B.  Reproduced: the ordered dither and
 * per-depth bit split of msf_cook_frame (vector body and scalar tail give the same values), the depth chain from frame to frame
 * (start at min(max_bit_depth, previous depth + 160 / max(1, previous count)), down while >= 256 colours are used), the palette in
 * ascending cooked value with bit replication, "unchanged pixel -> index 0" between frames of one bit split, disposal 0x09 in the
 * block in front of a frame with transparent pixels, the greedy LZW parse with its reset at 4096 entries and its capped final widths.
 * max_bit_depth is clamped to 1..16 as the reference clamps it; the delay keeps its low 16 bits.  saveGIF itself passes 7
 * centiseconds, depth 16 and the alpha threshold 10.
 * Deliberate deviations: a width or height below 1 or above 65535 (the reference writes truncated 16-bit fields), frames < 1, and a
 * shape with width * height * 4 > INT_MAX (the reference's int sizes wrap) are refused.
 * gamut_hip_gif_encode_bound: the reference's own reservation, 32 + frames * (32 + 768 + width * height * 3 / 2 + 256) + 1, which no
 * file exceeds; 0 when the shape is refused. */
int64_t gamut_hip_gif_encode_bound(int width, int height, int frames);
/* batch: animation i has frames[i] rgba8 layers in DEVICE memory, layer l at src[i] + l * src_layer_offset[i], rows src_pitch[i]
 * apart (negative allowed, any alignment), and is written to out + out_offset[i] (device, any alignment), which must have
 * gamut_hip_gif_encode_bound(...) bytes; nothing outside [out_offset[i], out_offset[i] + out_len[i]) is written.  centiseconds,
 * max_bit_depth, alpha_threshold: per animation, each array may be NULL (7, 16, 10).  out_len[i] / status_host[i] (host arrays;
 * status_host may be NULL): a refused animation (or a NULL src[i], a negative out_offset[i]) gets GAMUT_HIP_ERR_INVALID_ARG and
 * out_len 0, the others are still encoded, and the call returns the status of the lowest-numbered refused one.  Five launches and one
 * wait per call whatever the frame counts (the frame-to-frame depth chain is walked on the device).  Returns when the encode has
 * finished.  Working memory: the calling thread keeps, per device and for its lifetime like the library's other staging buffers
 * (grown on demand, never shrunk), the largest scratch a call of its has needed -- one block slot of 32 + 768 + width * height * 3 / 2
 * + 256 bytes and 16.4 KB of census bitmaps per frame of the batch (0.8 GB for 256 animations x 16 frames of 480 x 270);
 * gamut_hip_gif_write_to_mem and the Image layer's GIF save keep a staging buffer of pixels + bound bytes each in the same way. */
int     gamut_hip_gif_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const int64_t* src_layer_offset,
                                          const int32_t* width, const int32_t* height, const int32_t* frames,
                                          const int32_t* centiseconds, const int32_t* max_bit_depth, const int32_t* alpha_threshold,
                                          int count, const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host,
                                          void* stream);
/* host pixels (layer l at data + l * layer_offset, rows `pitch` bytes apart, negative allowed) through pinned staging -> malloc'd
 * file of *out_len bytes, or NULL on refusal (see last_error) */
void*   gamut_hip_gif_write_to_mem(const void* data, int pitch, int64_t layer_offset, int w, int h, int frames, int centiseconds,
                                   int max_bit_depth, int alpha_threshold, int* out_len);
/* measurements: with GAMUT_HIP_GIF_TIMING=1 the encode call brackets each of its kernels with events; this returns the GPU
 * milliseconds of kernel `which` of the calling thread's last encode call -- 0: colour census, 1: depth plan, 2: LZW, 3: block
 * offsets, 4: gather --, -1 when timing is off, nothing was encoded or `which` is out of range */
float gamut_hip_gif_last_encode_kernel_ms(int which);

/* ---- TGA (TGADecoder / TGAEncoder, codecs/tga.d; loadTGA / detectTGA / saveTGA, plugins/tga.d) -----------------------------------
 * Decode: every pixel what TGADecoder.decodeImage gives, bit for bit: image types 1 / 2 / 3 and their run-length forms 9 / 10 / 11, 8 / 15 /
 * 16 / 24 / 32 bits per pixel, colour maps of 8 / 15 / 16 / 24 / 32-bit entries under 8- or 16-bit indices, either row order.  Kept
 * from the reference: the colour map is reached by skipping palette_start BYTES (not entries); 15 / 16-bit pixels and colour-map
 * entries are (v * 255) / 31 per channel and are not R/B swapped; 16-bit grey is two raw bytes; a colour-map index >= palette_len
 * reads entry 0; run-length packets may cross row ends and the last one may overrun width * height (the surplus is dropped); the
 * descriptor's alpha bits and x-origin bit are ignored, and so is anything behind the pixels.  A read past the end of the file fails
 * (memory stream, io.d); a skip to exactly the end succeeds.
 * Deliberate deviation: width * height * components > 2^31 - 1 (components: the file's or, if larger, the requested ones) is refused;
 * the reference's `int` pixel offsets wrap there.
 * (Declared typedef-first: the layout of this struct is pinned by tests/c/tga_abi_layout.c and tests/test_tga_cpu.py.) */
typedef struct gamut_hip_tga_info gamut_hip_tga_info;
struct gamut_hip_tga_info {
    int32_t width, height;
    int32_t bpp;                    /* bits per pixel of the file: the index size when indexed */
    int32_t image_type;             /* 1, 2 or 3: the file's type after the - 8 of the run-length forms */
    int32_t rle, indexed, rgb16;    /* 0 / 1 each; rgb16: pixels (or colour-map entries) are 5-5-5 words */
    int32_t channels_in_file;       /* 1..4: l8, la8, rgb8, rgba8 (stbi__tga_get_comp of the cmap size when indexed, else of bpp) */
    int32_t bottom_up;              /* 1: the file's first row is the bottom one (descriptor bit 5 clear) */
    int32_t palette_start, palette_len, cmap_size;   /* 0 when the file has no colour map */
    int32_t data_offset;            /* 18 + ID length: where the colour map (after palette_start more bytes) or the pixels begin */
    int32_t detected;               /* 1: getImageInfo accepts bytes 0..16 (detectTGA), whatever the load verdict is */
};
/* the header alone (host, no GPU needed).  Two verdicts: info->detected is detectTGA's (the first 17 bytes), the return value is
 * the load's -- GAMUT_HIP_OK, or GAMUT_HIP_ERR_DECODE where getImageInfo or the header part of decodeImage refuse (descriptor byte
 * or ID field missing, too large).  Fields are filled as far as the header was read. */
int gamut_hip_tga_read_header(const uint8_t* data, size_t len, gamut_hip_tga_info* info);
/* `count` TGA files in host memory -> tight top-down rows of width * comps bytes at out + out_offset[i] (device).  req_comp 0: the
 * file's own components, decodeImage's bytes; 3 / 4: what convertTo(rgb8 / rgba8) makes of them (grey replicated, a missing alpha
 * 255, alpha dropped); anything else is GAMUT_HIP_ERR_INVALID_ARG.  Two launches for the whole batch (one over the unpacked
 * files, one over the run-length ones), whatever count, geometries and variants.  info[i] / status_host[i] (either may be NULL) per
 * file; a refused file gets GAMUT_HIP_ERR_DECODE and does not disturb the others; returns the status of the lowest-numbered refused
 * file.  Unpacked files and colour maps that the file is too short for are refused on the host and write nothing; a run-length stream
 * that ends before width * height pixels is refused on the device and may leave anything inside that image's own width * height *
 * comps bytes.  Nothing outside those bytes is written.  Returns when the pixels are in place. */
int gamut_hip_tga_decode_batch_device(const uint8_t* const* data, const size_t* len, int count, int req_comp,
                                      const int64_t* out_offset, uint8_t* out, gamut_hip_tga_info* info, int* status_host, void* stream);
/* the run-length kernel walks the packet stream in windows of this many bytes, counted from the first packet byte */
int   gamut_hip_tga_rle_window(void);
/* measurements: with GAMUT_HIP_TGA_TIMING=1 the decode call brackets its kernels (not the upload) with events; this returns the GPU
 * milliseconds of the calling thread's last decode call, -1 when timing is off or nothing was decoded */
float gamut_hip_tga_last_decode_kernel_ms(void);
/* Encode: byte for byte TGAEncoder (codecs/tga.d:57-281) as saveTGA drives it (plugins/tga.d:128-150) -- 18 header bytes (type 10
 * run-length or 2 raw, 24 or 32 bits, descriptor 0: rows bottom-up, no footer), B and R swapped, and with rle the reference's packets
 * row by row.  comp is the SOURCE's channel count: 1 = l8 and 3 = rgb8 give 3 file channels (grey replicated), 2 = la8 and 4 = rgba8
 * give 4.  Deliberate deviations: the reference refuses only a dimension above 65535 and the other pixel types; width or height 0 and
 * a bound above 2^31 - 1 are refused here too.
 * The most bytes a file can have, 18 + width * height * (file channels + 1) (reached at width 1), or 0 when the image is refused:
 * width or height outside 1..65535, comp outside 1..4, a bound above 2^31 - 1. */
int64_t gamut_hip_tga_encode_bound(int width, int height, int comp);
/* batch: image i is read from DEVICE memory at src[i] (rows src_pitch[i] apart, negative allowed, any alignment) and written to
 * out + out_offset[i] (device, any alignment), which must have gamut_hip_tga_encode_bound(...) bytes; nothing outside
 * [out_offset[i], out_offset[i] + out_len[i]) is written.  rle: 0 / 1 per image, NULL for 1 everywhere (saveTGA's choice).
 * out_len[i] / status_host[i] (host arrays; status_host may be NULL) are filled when the call returns: a refused image (or a NULL
 * src[i], a negative out_offset[i]) gets GAMUT_HIP_ERR_INVALID_ARG and out_len 0, the others are still encoded, and the call returns
 * the status of the lowest-numbered refused image.  Three launches, whatever the batch holds. */
int     gamut_hip_tga_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const int32_t* width,
                                          const int32_t* height, const int32_t* comp, const int32_t* rle, int count,
                                          const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host, void* stream);
/* host pixels (rows `pitch` bytes apart, negative allowed) through pinned staging -> malloc'd file of *out_len bytes, or NULL on
 * refusal (see last_error) */
void*   gamut_hip_tga_write_to_mem(const void* data, int pitch, int w, int h, int comp, int rle, int* out_len);
/* the encoder assembles a row's packets this many pixels at a time (a row wider than this is written in several pieces) */
int     gamut_hip_tga_encode_window(void);
/* measurements, under GAMUT_HIP_TGA_TIMING=1 as the decode getter: the GPU milliseconds of the calling thread's last encode call --
 * all three launches, or one of them (0 row lengths, 1 offsets, 2 write); -1 when timing is off or nothing was encoded */
float   gamut_hip_tga_last_encode_kernel_ms(void);
float   gamut_hip_tga_last_encode_stage_ms(int stage);

/* ---- SQZ decode (SQZ_decode, codecs/sqz.d; loadSQZ / detectSQZ, plugins/sqz.d) ----------------------------------------------------
 * SQZ is an embedded wavelet coder: a 6-byte header, then ONE bit stream that may be cut anywhere (every prefix of at least 7 bytes
 * of a good file is a good file).  The decoder has two halves.  The FRONT END (host threads, gamut_hip_sqz_decode_coeffs) walks the
 * bit stream -- WDR bit planes over linked lists per subband, interleaved by a schedule -- and leaves the reference's coefficient
 * buffer as it stands after SQZ_decode_round_coefficients.  The BACK END (HIP kernels, gamut_hip_sqz_reconstruct_batch_device) is
 * SQZ_dwt_convert_from_sign_magnitude, SQZ_idwt (up to eight levels of the in-place 5/3 integer IDWT per plane) and one of the four
 * inverse colour transforms (grey, YCoCg-R, integer Oklab, LOG-L1), bit for bit.  Encoding (saveSQZ) is the next section.
 * Refusals the reference does not have: an allocation that cannot be had (GAMUT_HIP_ERR_OUT_OF_MEMORY).  Nothing else deviates.
 * (Declared typedef-first: the layout of both structs is pinned by tests/c/sqz_abi_layout.c and tests/test_sqz_cpu.py.) */
typedef struct gamut_hip_sqz_info gamut_hip_sqz_info;
struct gamut_hip_sqz_info {
    int32_t width, height;          /* 8..65535 each */
    int32_t planes;                 /* 1 (colour mode 0) or 3 */
    int32_t color_mode;             /* 0 grey, 1 YCoCg-R, 2 Oklab, 3 LOG-L1 */
    int32_t levels;                 /* 1..8 DWT levels, at most ilog2(min side) - 3 with ilog2 = index of the top bit + 1 */
    int32_t scan_order;             /* 0 raster, 1 snake, 2 Morton, 3 Hilbert */
    int32_t subsampling;            /* 0 / 1: chroma planes scheduled one round later */
    int32_t pixel_type;             /* PixelType of the decoded image: 0 = l8, 9 = rgb8 */
    int32_t detected;               /* detectSQZ's verdict: the first byte is 0xA5 */
};
/* one image of a reconstruction batch */
typedef struct gamut_hip_sqz_desc gamut_hip_sqz_desc;
struct gamut_hip_sqz_desc {
    int32_t width, height, color_mode, levels;   /* as in gamut_hip_sqz_info; planes follows from color_mode */
    int64_t coeff_offset;           /* where this image's planes begin in `coeffs`, counted in int16 elements, >= 0 */
};
/* the header alone (host, no GPU needed): GAMUT_HIP_OK, or GAMUT_HIP_ERR_DECODE where SQZ_decode_header / SQZ_validate_input refuse
 * (wrong magic, fewer than 7 bytes, a side outside 8..65535, more levels than the size admits).  Fields are filled on success;
 * `detected` always. */
int gamut_hip_sqz_read_header(const uint8_t* data, size_t len, gamut_hip_sqz_info* info);
/* the front end (host, no GPU needed): planes * width * height coefficients exactly as the reference holds them after
 * SQZ_decode_round_coefficients -- sign-magnitude, bit 0 the sign, planes one after another, subbands interleaved in place -- into
 * planes[0 .. capacity).  A capacity below planes * width * height is GAMUT_HIP_ERR_INVALID_ARG (info is filled: ask with capacity 0). */
int gamut_hip_sqz_decode_coeffs(const uint8_t* data, size_t len, int16_t* planes, size_t capacity, gamut_hip_sqz_info* info);
/* the back end: `count` images whose coefficient planes are resident in device memory at coeffs + descs[i].coeff_offset ->
 * tight rows of width * planes bytes (l8 or rgb8) at out + out_offset[i] (device, any byte alignment).  descs, out_offset and
 * status_host are host arrays; status_host may be NULL.  `coeffs` is a WORKING buffer: its contents after the call are unspecified.
 * An image whose desc is refused (geometry that gamut_hip_sqz_read_header would refuse, a negative offset) gets
 * GAMUT_HIP_ERR_INVALID_ARG and writes nothing, the others are reconstructed, and the call returns the status of the lowest-numbered
 * refused image ("image %d: ...").  One launch per DWT level -- as many as the deepest image of the batch has, at most eight,
 * whatever the number of images; the last one does the colour transform as well.  Nothing outside an image's own width * height *
 * planes bytes is written.  Returns when the pixels are in place. */
int gamut_hip_sqz_reconstruct_batch_device(const int16_t* coeffs, const gamut_hip_sqz_desc* descs, int count, const int64_t* out_offset,
                                           uint8_t* out, int* status_host, void* stream);
/* `count` SQZ files in host memory -> pixels as above.  Headers are parsed, the front end runs on the library's host worker pool (at
 * most 16 threads), the coefficients are staged in pinned memory and uploaded, the back end follows.  info[i] / status_host[i] (host
 * arrays, either may be NULL) are filled when the call returns; a refused file gets GAMUT_HIP_ERR_DECODE and writes nothing, its
 * neighbours are decoded, and the call returns the status of the lowest-numbered refused file ("image %d: ..."). */
int gamut_hip_sqz_decode_batch_device(const uint8_t* const* data, const size_t* len, int count, const int64_t* out_offset, uint8_t* out,
                                      gamut_hip_sqz_info* info, int* status_host, void* stream);
/* SQZ_linear_to_sRGB (codecs/sqz.d:1287-1321): 512 bytes, generated from the sRGB transfer function (every entry reproduced) */
const uint8_t* gamut_hip_sqz_linear_to_srgb_table(void);
/* measurements: with GAMUT_HIP_SQZ_TIMING=1 the calls bracket their stages with events / clocks; milliseconds of the calling thread's
 * last call -- 0: the back end's kernels (GPU time), 1: the host front end of the file-level call (wall clock), 2: staging copy and
 * upload (wall clock until the upload is queued); -1 when timing is off, nothing was decoded or `stage` is out of range */
float gamut_hip_sqz_last_decode_stage_ms(int stage);

/* ---- SQZ read on the device (SQZ_schedule_task's read side, codecs/sqz.d:1941-2168, as HIP kernels) ------------------------------
 * The front end again, without the host threads: one workgroup per file walks the chain of (band, bit plane) segments and spends all
 * its lanes inside each -- flags by parity, records ranked and their advances summed by workgroup prefix sums, the first run past the
 * list found by a minimum (gamut_amd/csrc/sqz_read.hip; the rules by bit position are in sqz_read.hpp).  The files are in HOST
 * memory and go up through pinned staging; file i's planes * width * height int16 coefficients land in DEVICE memory at coeffs +
 * coeff_offset[i] (int16 elements, >= 0), value for value what gamut_hip_sqz_decode_coeffs writes -- the buffer behind
 * SQZ_decode_round_coefficients, ready for gamut_hip_sqz_reconstruct_batch_device.  data, len, coeff_offset, info and status_host
 * are host arrays; info and status_host may be NULL.  The header's refusals are the host's: a refused file (or a negative
 * coeff_offset[i]) writes nothing, its neighbours are read, and the call returns the status of the lowest-numbered refused file
 * ("image %d: ...").  Nothing outside a file's own coefficients is written.  Returns when they are in place. */
int gamut_hip_sqz_read_batch_device(const uint8_t* const* data, const size_t* len, int count, int16_t* coeffs, const int64_t* coeff_offset,
                                    gamut_hip_sqz_info* info, int* status_host, void* stream);
/* Which front end gamut_hip_sqz_decode_batch_device and the Image layer's SQZ load run behind their unchanged signatures: 0 the host
 * front end, 1 the device reader (no coefficient crosses the bus; gamut_hip_sqz_last_decode_stage_ms then gives -1 for stages 1 and
 * 2).  Returns the previous value; any other argument changes nothing.  Process-wide; the initial value is
 * GAMUT_HIP_SQZ_READER=host|device from the environment, default host. */
int gamut_hip_sqz_set_reader(int which);
/* the bits of a sorting pass the device reader's workgroup takes per step (tests size their cases around it) */
int gamut_hip_sqz_read_window(void);
/* The device reader takes a batch in chunks of files that have at most this many coefficients between them (its lists are 8 bytes
 * per coefficient; one larger file is a chunk of its own).  Sets the limit and returns the previous one; a value below 1 changes
 * nothing.  Process-wide. */
int64_t gamut_hip_sqz_set_read_chunk(int64_t coefficients);
/* measurements, under GAMUT_HIP_SQZ_TIMING=1: milliseconds of the calling thread's last call that ran the device reader -- 0: its
 * kernels (GPU time, all chunks), 1: building the band tables, staging the files and queueing the upload (wall clock); -1 otherwise */
float gamut_hip_sqz_last_read_stage_ms(int stage);

/* ---- SQZ encode (SQZ_encode, codecs/sqz.d:2208-2240; saveSQZ, plugins/sqz.d:141-201) -----------------------------------------------
 * The decoder's split, mirrored.  The FRONT HALF (HIP kernels, gamut_hip_sqz_analyze_batch_device) is SQZ_color_process(read = 1) for
 * the four colour modes, SQZ_dwt (the in-place 5/3 integer DWT, one launch per level over the whole batch) and
 * SQZ_dwt_convert_to_sign_magnitude, bit for bit -- the horizontal pass's untruncated running ints and every 16-bit wrap included --
 * and ends with the reference's coefficient buffer in device memory, exactly what gamut_hip_sqz_reconstruct_batch_device consumes.
 * The BACK HALF (host threads, gamut_hip_sqz_encode_coeffs) is SQZ_encode_header and SQZ_schedule_task over SQZ_encode_init_subband /
 * SQZ_encode_bitplane: the embedded bit-plane writer, cut at the byte budget.
 * Deviations: (1) a subband in which EVERY sign-magnitude value is a negative short (every |coefficient| >= 16384) is refused with
 * GAMUT_HIP_ERR_INVALID_ARG: the reference takes the maximum as a signed short, gets bit plane 32 from it and shifts 1u by 32, which
 * is not defined.  A band with at least one smaller value is written as the reference writes it (the large values' top bit is not
 * seen).  8-bit pixels cannot produce either.  (2) An allocation that cannot be had is GAMUT_HIP_ERR_OUT_OF_MEMORY.
 * (Declared typedef-first: the layout is pinned by tests/c/sqz_encode_abi_layout.c and tests/test_sqz_encode_cpu.py.) */
typedef struct gamut_hip_sqz_encode_desc gamut_hip_sqz_encode_desc;
struct gamut_hip_sqz_encode_desc {
    int32_t width, height;          /* 8..65535 each */
    int32_t color_mode;             /* 0 grey (l8 pixels, one plane), 1 YCoCg-R, 2 Oklab, 3 LOG-L1 (rgb8 pixels, three planes) */
    int32_t levels;                 /* 1..8; more than ilog2(min side) - 3 is CLAMPED to that, as SQZ_validate_input(read_only = 0) does */
    int32_t scan_order;             /* 0 raster, 1 snake, 2 Morton, 3 Hilbert */
    int32_t subsampling;            /* 0 / not 0: chroma planes scheduled one round later */
    int64_t budget;                 /* bytes the file may take, header included; the analysis entries do not look at it */
};
/* saveSQZ's budget, to the letter: bpp8 = (flags >> 5) & 0xff, 0 meaning 0x50; bpp = bpp8 / 32.0f widened to double;
 * 6 + (int64)((double)width * height * bpp / 8.0) */
int64_t gamut_hip_sqz_budget_from_flags(int width, int height, int flags);
/* the front half: `count` images resident in device memory, l8 (colour mode 0) or rgb8, rows src_pitch[i] bytes apart (padded or
 * negative, any byte alignment; exactly width * planes bytes of a row are read) -> planes * width * height int16 coefficients per
 * image at coeffs + coeff_offset[i] (device, counted in int16 elements, >= 0): sign-magnitude with bit 0 the sign, planes one after
 * another, subbands interleaved in place (SQZ_common_init_context).  src, src_pitch, descs, coeff_offset and status_host are host
 * arrays; status_host may be NULL.  An image whose desc is refused (a side outside 8..65535, a mode or scan order outside 0..3,
 * levels outside 1..8, a NULL src[i], a negative offset) gets GAMUT_HIP_ERR_INVALID_ARG and writes nothing, the others are done, and
 * the call returns the status of the lowest-numbered refused image ("image %d: ...").  One launch per DWT level, shallowest first --
 * at most eight whatever the number of images; the first does the colour transform in its load, every one converts to
 * sign-magnitude in its stores.  Nothing outside an image's own coefficients is written.  Returns when they are in place. */
int gamut_hip_sqz_analyze_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const gamut_hip_sqz_encode_desc* descs, int count,
                                       int16_t* coeffs, const int64_t* coeff_offset, int* status_host, void* stream);
/* the same level kernels fed with two's-complement int16 planes in raster order, planes one after another, at planes_in +
 * coeff_offset[i] (device; must not overlap `coeffs`): SQZ_dwt and SQZ_dwt_convert_to_sign_magnitude alone, the exact inverse of
 * what gamut_hip_sqz_reconstruct_batch_device does before its colour stage.  color_mode only gives the plane count.  This is the
 * way to values no 8-bit pixel produces. */
int gamut_hip_sqz_dwt_batch_device(const int16_t* planes_in, const gamut_hip_sqz_encode_desc* descs, int count, int16_t* coeffs,
                                   const int64_t* coeff_offset, int* status_host, void* stream);
/* the back half (host, no GPU needed), the mirror of gamut_hip_sqz_decode_coeffs: header and bit planes of the coefficient buffer
 * `planes` (as the front half leaves it) into dst[0 .. desc->budget), which is cleared first as saveSQZ clears it; *len = (bits used
 * + 7) / 8.  levels is clamped as above.  A budget of at most 6 bytes is GAMUT_HIP_ERR_INVALID_ARG before anything is written (the
 * reference's SQZ_BUFFER_TOO_SMALL: the header's verdict is !eob after its last bit).  On a refusal *len is 0 and dst[0 .. budget)
 * is unspecified. */
int gamut_hip_sqz_encode_coeffs(const int16_t* planes, const gamut_hip_sqz_encode_desc* desc, uint8_t* dst, int64_t* len);
/* device pixels -> files: the front half, ONE download of the batch's coefficients into pinned staging, the back half on the
 * library's host worker pool (one image per thread, at most 16 threads).  `out` is HOST memory: by default the writer runs on the
 * host.  (With gamut_hip_sqz_set_writer(1) the device writer of the next section runs instead and only the files are downloaded;
 * gamut_hip_sqz_encode_batch_to_device leaves them in device memory.)  File i goes to out + out_offset[i],
 * where descs[i].budget bytes must be writable; out_len[i] (host) is its length, 0 for a refused image.  Nothing outside
 * [out_offset[i], out_offset[i] + out_len[i]) is written.  Refusals and the returned status as for the front half; a budget of at
 * most 6 bytes and deviation (1) are refusals too. */
int gamut_hip_sqz_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const gamut_hip_sqz_encode_desc* descs, int count,
                                      const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host, void* stream);
/* the host drop-in for SQZ_encode: pixels in host memory (rows `pitch` bytes apart, may be negative) go up through pinned staging,
 * the call above follows; the file comes back in malloc memory (*out_len bytes, free()), or NULL with the thread's message */
void* gamut_hip_sqz_write_to_mem(const void* data, int pitch, const gamut_hip_sqz_encode_desc* desc, int* out_len);
/* measurements, under the decoder's GAMUT_HIP_SQZ_TIMING=1: milliseconds of the calling thread's last call -- 0: the front half's
 * kernels (GPU time), 1: the host writer (wall clock), 2: download and staging (wall clock); -1 otherwise */
float gamut_hip_sqz_last_encode_stage_ms(int stage);

/* ---- SQZ write on the device (SQZ_schedule_task, codecs/sqz.d:1866-2168, as HIP kernels) ------------------------------------------
 * The back half again, without the host: every (band, bit plane) segment of the embedded stream is a pure function of the band's
 * coefficients in scan order, the order of the segments depends on the bands' maxima alone, and the file is the first 8 * budget
 * bits of their concatenation -- counts, prefix sums and bit packing at computed offsets (gamut_amd/csrc/sqz_write.hip; six launches
 * per chunk of images).  No coefficient crosses the bus: 16 bytes per image come down mid-call.  The files are byte for byte those of
 * gamut_hip_sqz_encode_coeffs, and so are the verdicts: levels clamped, a budget of at most 6 bytes refused, deviation (1) refused
 * exactly when the schedule reaches the band of nothing but negative shorts before the budget is spent.
 *
 * coeffs: DEVICE memory, image i's buffer at coeffs + coeff_offset[i] (int16 elements) as gamut_hip_sqz_analyze_batch_device leaves
 * it; only read.  File i goes to out + out_offset[i] (DEVICE memory, any alignment), where descs[i].budget bytes must be writable;
 * nothing outside [out_offset[i], out_offset[i] + out_len[i]) is written.  coeff_offset, descs, out_offset, out_len and status_host
 * (may be NULL) are host arrays.  A refused image writes nothing and gets out_len 0, the others are written, and the call returns the
 * status of the lowest-numbered refused image ("image %d: ..."); it returns when the files are in place. */
int gamut_hip_sqz_write_batch_device(const int16_t* coeffs, const int64_t* coeff_offset, const gamut_hip_sqz_encode_desc* descs, int count,
                                     const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host, void* stream);
/* device pixels -> files in DEVICE memory: the front half, then the call above.  The arguments are those of
 * gamut_hip_sqz_encode_batch_device, except that `out` is device memory. */
int gamut_hip_sqz_encode_batch_to_device(const uint8_t* const* src, const int64_t* src_pitch, const gamut_hip_sqz_encode_desc* descs, int count,
                                         const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host, void* stream);
/* a band's scan (host, no GPU needed): the width * height (x, y) pairs, 2 * width * height uint16, in the order SQZ_scan_init's
 * scanner visits them -- order 0 raster, 1 snake (tile 4 x 15), 2 Morton, 3 Hilbert.  These are the tables the device writer uploads.
 * GAMUT_HIP_ERR_INVALID_ARG for an order outside 0..3, a side below 1 or above 65535, or a NULL xy. */
int gamut_hip_sqz_scan_order(int order, int width, int height, uint16_t* xy);
/* the coefficients a wave of the device writer takes per step of its walk over a band (tests size their cases around it) */
int gamut_hip_sqz_write_chunk(void);
/* measurements, under GAMUT_HIP_SQZ_TIMING=1: milliseconds of the calling thread's last call that ran the device writer -- 0: its
 * kernels (GPU time, all chunks), 1: building the band and scan tables (wall clock); -1 otherwise */
float gamut_hip_sqz_last_write_stage_ms(int stage);
/* Which writer gamut_hip_sqz_encode_batch_device, gamut_hip_sqz_write_to_mem and the Image layer's SQZ save run behind their
 * unchanged signatures: 0 the host writer, 1 the device writer (the files alone are downloaded; gamut_hip_sqz_last_encode_stage_ms
 * then gives -1 for stages 1 and 2).  Returns the previous value; any other argument changes nothing.  Process-wide; the initial
 * value is GAMUT_HIP_SQZ_WRITER=host|device from the environment, default host. */
int gamut_hip_sqz_set_writer(int which);

/* ---- DDS / BC7 encode (saveDDS, plugins/dds.d:47-216; bc7enc16_compress_block, codecs/bc7enc16.d) --------------------------------
 * The file saveDDS writes, byte for byte: "DDS ", DDSURFACEDESC2, DDS_HEADER_DXT10 (148 bytes, DXGI_FORMAT_BC7_UNORM), then one
 * 16-byte BC7 block per 4 x 4 tile in row-major order, each what bc7enc16_compress_block gives on the parameters of
 * bc7enc16_compress_block_params_init (64 mode-1 partitions, least squares, partition filterbank, uber level 0, perceptual weights):
 * mode 6, or mode 1 for an opaque tile where it has the smaller error.  comp is the source's channel count: 1 (l8) -> (v, v, v, 255),
 * 2 (la8) -> (v, v, v, a), 3 (rgb8) -> (r, g, b, 255), 4 (rgba8); a tile position outside the image is (0, 0, 0, 0), as the
 * reference's zero-initialised tile has it.  The reference only writes this format; nothing here reads it.
 * Deliberate deviation: the reference's `int numBlocks` wraps for huge images; a file above 2^31 - 1 bytes is refused here.
 * The file's size, 148 + 16 * ((width + 3) / 4) * ((height + 3) / 4), or 0 when the image is refused: width or height below 1,
 * comp outside 1..4, a size above 2^31 - 1. */
int64_t gamut_hip_dds_encode_bound(int width, int height, int comp);
/* batch: image i is read from DEVICE memory at src[i] (rows src_pitch[i] apart, negative allowed, any alignment) and written to
 * out + out_offset[i] (device, any alignment), which must have gamut_hip_dds_encode_bound(...) bytes; nothing outside
 * [out_offset[i], out_offset[i] + out_len[i]) is written.  out_len[i] / status_host[i] (host arrays; status_host may be NULL) are
 * filled when the call returns: a refused image (or a NULL src[i], a negative out_offset[i]) gets GAMUT_HIP_ERR_INVALID_ARG and
 * out_len 0, the others are still encoded, and the call returns the status of the lowest-numbered refused image.  One launch,
 * whatever the batch holds: a tile is 16 lanes' work and a workgroup serves tiles of any image. */
int     gamut_hip_dds_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const int32_t* width,
                                          const int32_t* height, const int32_t* comp, int count, const int64_t* out_offset,
                                          uint8_t* out, int64_t* out_len, int* status_host, void* stream);
/* the codec without the container: n tiles of 16 rgba pixels (64 bytes each, DEVICE, any alignment; pixel i of a tile is column
 * i % 4 of row i / 4) -> n blocks of 16 bytes each (DEVICE, any alignment); n <= 2^31 - 1.  Like the batch call it returns when
 * the stream has finished the work. */
int     gamut_hip_bc7_encode_blocks_device(const uint8_t* rgba_tiles, int64_t n, uint8_t* out, void* stream);
/* host pixels (rows `pitch` bytes apart, negative allowed) through pinned staging -> malloc'd file of *out_len bytes, or NULL on
 * refusal (see last_error) */
void*   gamut_hip_dds_write_to_mem(const void* data, int pitch, int width, int height, int comp, int* out_len);
/* measurements, under GAMUT_HIP_DDS_TIMING=1: the GPU milliseconds of the launch of the calling thread's last dds_encode_batch_device
 * or bc7_encode_blocks_device call; -1 when timing is off or nothing was encoded */
float   gamut_hip_dds_last_encode_kernel_ms(void);

/* ---- QOIX, 8-bit rgb / rgba (qoix_lz4_decode, plugins/qoix.d:350-473; LZ4_decompress_fast, codecs/lz4.d:760-978; qoix_decode,
 * codecs/qoi2avg.d:624-897) ------------------------------------------------------------------------------------------------------
 * Decode: every pixel what the reference gives, bit for bit, for files that hold 8-bit rgb or rgba (what saveQOIX writes for rgb8,
 * rgba8 and rgbap8), stored or LZ4-compressed.  Kept from the reference: the load flags are only validated and the decoder produces
 * the file's own channel count; the last four bytes are never decoded as opcodes and never checked; a stream that ends early repeats
 * the last pixel and surplus ops are ignored; runs cross row ends and are cut at the image's end; a 3-channel file may carry ADIFF
 * and RGBA ops, whose alpha shows when 4 channels are asked for; whatever follows the LZ4 block's final literal run is ignored.
 * The 10-bit codecs are not built yet: GAMUT_HIP_ERR_UNSUPPORTED.  The grey codec (8-bit with 1 or 2 channels: QOI-Plane,
 * qoiplane_decode, codecs/qoiplane.d:377-541) is built behind the process-wide switch gamut_hip_qoix_set_plane, whose default keeps
 * such files GAMUT_HIP_ERR_UNSUPPORTED.  With the switch on they decode to l8 / la8 (lap8 never: QOI-Plane refuses colorspace 2), bit
 * for bit.  Kept from the reference there: the closing four bytes ARE decoded (f ff is "repeat to the end", which is how a stream
 * ends); a stream that ends that way early repeats the last pixel; surplus ops are ignored; runs cross row ends; a DIRECT in a
 * 2-channel file sets luminance only; 1 channel asked of a 2-channel file drops alpha, 2 asked of a 1-channel file gives 255 unless
 * ADIFF / LA ops set it.
 * Deliberate deviations, each where the reference touches memory it does not own, each GAMUT_HIP_ERR_DECODE:
 *   1. LZ4: any read at or past the end of the file refuses the file (the reference has no input bound);
 *   2. LZ4: offset 0, or a match that starts before the first output byte, refuses the file (the reference reads up to 64 KiB in
 *      front of its buffer);
 *   3. QOI2AVG: an END opcode that is executed refuses the file (the reference leaves the rest of the row as whatever its scanline
 *      buffer held, uninitialised memory in rows 0 and 1); no valid file executes END;
 *   4. QOI2AVG: an op byte read at index >= size refuses the file (an ADIFF chain running through the last four bytes);
 *  P1. QOI-Plane: a nibble read at byte index >= size refuses the file (the reference has no input bound).
 * Also refused: a length above INT_MAX (loadQOIX keeps it in an int), and an `orig` above 255 * (length - 29), which no LZ4 block
 * of that length can produce (it could only end in deviation 1).
 * (Declared typedef-first: the layout of this struct is pinned by tests/c/qoix_abi_layout.c and tests/test_qoix_cpu.py.) */
typedef struct gamut_hip_qoix_info gamut_hip_qoix_info;
struct gamut_hip_qoix_info {
    int32_t width, height;          /* the header's big-endian u32 fields */
    int32_t version, channels, bitdepth, colorspace, compression;      /* bytes 12..16 */
    float   pixel_aspect_ratio;     /* bytes 17..20, bit for bit */
    float   resolution_y;           /* bytes 21..24, bit for bit: vertical DPI */
    int32_t orig;                   /* compression 1: the big-endian int at bytes 25..28; else 0 */
    int32_t pixel_type;             /* identifyTypeFromStream's GAMUT_PIXEL_* (rgbap8 for colorspace 2 with 4 channels), -1 when it refuses */
    int32_t detected;               /* 1: the file starts with "qoix" (detectQOIX), whatever the load verdict is */
};
/* the header alone (host, no GPU needed).  info->detected is detectQOIX's verdict, the return value the load's on everything that
 * is decidable without the body: GAMUT_HIP_OK, GAMUT_HIP_ERR_UNSUPPORTED for a header the container accepts but whose codec is not
 * built yet (bitdepth 10, or 8-bit with 1 or 2 channels while gamut_hip_qoix_set_plane is off), GAMUT_HIP_ERR_DECODE for a refusal.
 * Fields are filled as far as the header was read.  With the switch on an 8-bit 1- or 2-channel header goes through
 * qoiplane_decode's checks (QOI2AVG's, with colorspace <= 1: a 2-channel file of colorspace 2 has pixel_type lap8 and is refused). */
int gamut_hip_qoix_read_header(const uint8_t* data, size_t len, gamut_hip_qoix_info* info);
/* `count` QOIX files in host memory -> tight rows of width * channels bytes at out + out_offset[i] (device, any alignment).
 * channels 0: the file's own count; 3 / 4 as in qoix_decode (alpha dropped / kept, 255 unless ADIFF or RGBA ops set it); anything
 * else is GAMUT_HIP_ERR_INVALID_ARG (for 1 / 2 see gamut_hip_qoix_set_plane).  Two launches whatever a batch of colour files holds: one over the LZ4 files (a wave each; skipped when there
 * are none), one over all op streams (a wave each).  info[i] / status_host[i] (either may be NULL) per file; a failing file gets its
 * status and does not disturb the others; returns the status of the lowest-numbered failing file, whose number the tail of
 * last_error names ("image %d:").  A file refused on the host writes nothing; one refused on the device (the verdict is the
 * kernels' status word, not a host pre-walk) may leave anything inside its own width * height * channels bytes.  Nothing outside
 * those bytes is written.  The files go up through pinned staging; returns when the pixels are in place. */
int gamut_hip_qoix_decode_batch_device(const uint8_t* const* data, const size_t* len, int count, int channels,
                                       const int64_t* out_offset, uint8_t* out, gamut_hip_qoix_info* info, int* status_host, void* stream);
/* host drop-in with qoix_lz4_decode's argument list: the pixels (the file's own channel count, tight rows) in a malloc'd buffer and
 * *decoded_type = the stream's GAMUT_PIXEL_*, or NULL (flags that validLoadFlags refuses, a refused file, no device) */
void* gamut_hip_qoix_lz4_decode(const void* data, int size, gamut_hip_qoix_info* info, int flags, int* decoded_type);
/* the op-stream kernel keeps rows of up to this many pixels in LDS; a wider row lives in a global scratch row */
int   gamut_hip_qoix_row_capacity(void);
/* measurements: with GAMUT_HIP_QOIX_TIMING=1 the decode call brackets its kernels (not the upload) with events; the GPU milliseconds
 * of the calling thread's last decode call -- both kernels, or one (stage 0: LZ4, 1: op streams); -1 when timing is off, nothing was
 * decoded or `stage` is out of range */
float gamut_hip_qoix_last_decode_kernel_ms(void);
float gamut_hip_qoix_last_decode_stage_ms(int stage);
/* The QOI-Plane switch, process-wide: `on` is 0 or 1, the previous value is returned, any other argument changes nothing (and
 * returns the current value).  Initial value: GAMUT_HIP_QOIX_PLANE=0|1 in the environment, default 0.  Off, every QOIX entry behaves
 * as it did before the codec existed.  On, 8-bit files with 1 or 2 channels decode through every QOIX entry and Image.loadFromMemory;
 * gamut_hip_qoix_decode_batch_device then also takes channels 1 / 2, which apply to grey files as 3 / 4 apply to colour files: a file
 * of the other family gets GAMUT_HIP_ERR_INVALID_ARG as its status, writes nothing and does not disturb its neighbours (channels 0
 * suits a mixed batch).  Grey files run in a third launch, k_qoix_plane (a wave each), skipped when the batch holds none.
 * The switch means "the QOI-Plane codec is on" in both directions: on, the encode entries below take channels 1 / 2 as well. */
int   gamut_hip_qoix_set_plane(int on);
/* k_qoix_plane keeps rows of up to this many pixels in LDS; a wider row lives in a global scratch row */
int   gamut_hip_qoix_plane_row_capacity(void);
/* GPU milliseconds of k_qoix_plane in the calling thread's last decode call, under GAMUT_HIP_QOIX_TIMING=1 as the getters above (whose
 * values do not include it); -1 when timing is off or nothing was decoded */
float gamut_hip_qoix_last_plane_kernel_ms(void);
/* Encode: byte for byte qoix_lz4_encode (plugins/qoix.d:251-339) as saveQOIX drives it (:156-242) for 8-bit rgb / rgba -- the 25
 * header bytes, the op stream of qoix_encode (codecs/qoi2avg.d:376-615) with its four 0xff bytes, the LZ4 block of LZ4_compress on a
 * 64-bit build (codecs/lz4.d:289-554: byU16 below 65547 input bytes, byU32 from there) and the choice between the two files.  Kept
 * from the reference: px starts at (0, 0, 0, 255); runs cross row ends and end as RUN2 at 1024 pixels or at the last pixel, however
 * short; the index is a 1024-entry table of positions into a 64-entry FIFO, both zero at first, untouched by a hit; on a miss the
 * alpha step comes first (ADIFF and a colour op, or RGBA alone); LUMA, LUMA, GRAY, LUMA2, LUMA3, RGB are tried in that order.
 * Refused, as the reference does: width or height 0, channels outside 3..4, colorspace above 2, height >= 400000000 / width.
 * Deliberate deviations:
 *   1. for 4 channels the reference copies pitchBytes into a scanline buffer of 4 * width bytes (a padded pitch overruns it, a
 *      negative one is a huge memcpy); here width * channels bytes of every row are read, whatever the pitch is;
 *   2. the reference's int max_size wraps for large shapes; a description whose bound exceeds 2^31 - 1 is refused instead.
 * Grey, 1 or 2 channels, is QOI-Plane (qoiplane_encode, codecs/qoiplane.d:109-365) and exists while gamut_hip_qoix_set_plane is on; off,
 * such a description is refused as before the codec existed.  The state starts as {l: 0, a: 255}; a run is cut at 258 pixels, at the
 * last pixel and in front of a pixel that differs (REPEAT1 for 1..3, REPEAT2 above); an alpha step outside -7..7 is an LA, one inside
 * an ADIFF and a luminance op; the luminance op is the first of DIFF1, DIFF2, DIRECT that fits the difference to the rounded-up mean
 * of the pixel above (row 0: the predecessor) and the predecessor; nine f nibbles close the stream, one more ends it on a byte.
 * Colorspace 0..2 is written as given (saveQOIX writes 2 for lap8, which qoiplane_decode then refuses).  Deviations of the grey codec:
 *   G1. the reference allocates (w * h * n + 1) / 2 + 29 bytes (n = 3 or 6 nibbles a pixel), a byte too few when every pixel takes
 *       its worst op and w * h * n is even; the bound here is sized by the true maximum, datalen_max = (w * h * n + 10) / 2;
 *   G2. w * h * 6 above 2^31 - 1 (2 channels, more than 357913941 pixels) is refused: the reference's int size wraps there.
 * A batch may mix grey and colour images.  The 10-bit codecs are not built: refused.
 * (Declared typedef-first: the layout of this struct is pinned by tests/c/qoix_encode_abi_layout.c and tests/test_qoix_encode_cpu.py.) */
typedef struct gamut_hip_qoix_desc gamut_hip_qoix_desc;
struct gamut_hip_qoix_desc {
    int32_t width, height;
    int32_t channels;               /* 3 | 4, and 1 | 2 while gamut_hip_qoix_set_plane is on: the SOURCE's channel count, which is the file's */
    int32_t colorspace;             /* 0..2, header byte 15 (2: premultiplied alpha) */
    int32_t mode;                   /* 0: the reference's choice, LZ4 when lz4Size + 4 < datalen, else stored; 1: always stored (qoix_encode alone) */
    float   pixel_aspect_ratio;     /* header bytes 17..20, big-endian, bit for bit (NaN payloads included) */
    float   resolution_y;           /* header bytes 21..24, likewise */
};
/* the bytes a caller must provide for one file: with datalen_max = width * height * (channels + 1) + 4 (colour) or
 * (width * height * n + 10) / 2, n = 3 nibbles a pixel for 1 channel and 6 for 2 (grey), it is
 * 29 + datalen_max + datalen_max / 255 + 16 (the stored file and the LZ4 file at LZ4_compressBound); -1 for a refused description
 * (NULL, the reference's refusals, a mode other than 0 / 1, a bound above 2^31 - 1) */
int64_t gamut_hip_qoix_encode_bound(const gamut_hip_qoix_desc* desc);
/* batch: image i is read from DEVICE memory at src[i] (rows src_pitch[i] apart, padded or negative allowed, any alignment) and its
 * file written to out + out_offset[i] (device, any alignment), which must have gamut_hip_qoix_encode_bound(&descs[i]) bytes; nothing
 * outside [out_offset[i], out_offset[i] + out_len[i]) is written.  out_len[i] / status_host[i] (host arrays; status_host may be
 * NULL) are filled when the call returns: a refused image (or a NULL src[i], a negative out_offset[i]) gets
 * GAMUT_HIP_ERR_INVALID_ARG and out_len 0, the others are still encoded, and the call returns the status of the lowest-numbered
 * refused image ("image %d:" in last_error).  Three launches, whatever a batch of colour images holds: ops, LZ4, the choice.  Grey
 * images add three of their own, whatever they are -- k_qpenc_count and k_qpenc_write, a wave per segment of
 * gamut_hip_qoix_plane_encode_segment() pixels of the raster, and k_qpenc_scan between them -- and a batch without colour images
 * does not launch the colour op kernel. */
int     gamut_hip_qoix_encode_batch_device(const uint8_t* const* src, const int64_t* src_pitch, const gamut_hip_qoix_desc* descs, int count,
                                           const int64_t* out_offset, uint8_t* out, int64_t* out_len, int* status_host, void* stream);
/* host drop-in for qoix_lz4_encode: host pixels (rows `pitch` bytes apart, negative allowed) through pinned staging -> malloc'd file
 * of *out_len bytes, or NULL on refusal (see last_error) */
void*   gamut_hip_qoix_write_to_mem(const void* data, int pitch, const gamut_hip_qoix_desc* desc, int* out_len);
/* the op kernel takes this many pixels of the raster per step */
int     gamut_hip_qoix_encode_window(void);
/* the grey encoder cuts an image's raster into segments of this many consecutive pixels (a multiple of 64, whatever the width is) */
int     gamut_hip_qoix_plane_encode_segment(void);
/* LZ4_compressBound (n + n / 255 + 16; 0 for n < 0 or n > 0x7E000000), and LZ4_compress for `count` byte strings in DEVICE memory:
 * string i (src[i], len[i] bytes, any alignment) becomes the LZ4 block at out + out_offset[i], which must have
 * gamut_hip_lz4_compress_bound(len[i]) bytes; out_len[i] is the block's length, byte for byte what LZ4_compress writes on a 64-bit
 * build (a length of 0 gives the one-byte block 00).  Refusals (NULL src[i], a length out of range, a negative offset) as in the
 * image batch.  One launch, a wave per string. */
int     gamut_hip_lz4_compress_bound(int n);
int     gamut_hip_lz4_compress_batch_device(const uint8_t* const* src, const int32_t* len, int count, const int64_t* out_offset, uint8_t* out,
                                            int64_t* out_len, int* status_host, void* stream);
/* measurements, under GAMUT_HIP_QOIX_TIMING=1 as the decode getters: the GPU milliseconds of the calling thread's last encode call --
 * all three launches, or one of them (0 ops, 1 LZ4, 2 the choice); -1 when timing is off or nothing was encoded */
float   gamut_hip_qoix_last_encode_kernel_ms(void);
float   gamut_hip_qoix_last_encode_stage_ms(int stage);
/* likewise the grey encoder's three launches in the calling thread's last encode call (0 count, 1 scan, 2 write); -1 when timing is
 * off or that call encoded no grey image.  The getters above do not include them. */
float   gamut_hip_qoix_last_plane_encode_stage_ms(int stage);

/* ---- files of any of the three formats, one call ---------------------------------------------------------------------
 * The reference loads any file through Image.loadFromMemory: identifyFormatFromStream (image.d:1045-1061 -- the plugins' detect
 * procedures, a signature test each: plugins/jpeg.d:106-110, png.d:165-169, qoi.d:143-147) picks g_plugins[fif].loadProc
 * (image.d:1751-1772).  gamut_hip_identify_format is that test (GAMUT_HIP_FORMAT_*, the ImageFormat ordinals of types.d:14-21, or
 * GAMUT_HIP_FORMAT_UNKNOWN); gamut_hip_decode_batch_device takes `count` files of ANY of the three formats in host memory and
 * leaves rows of width * req_comps bytes (req_comps = 3 / 4: rgb8 / rgba8, what all three decoders produce; 16-bit PNG samples
 * are reduced as stbi_load does) at out + out_offset[i] (device) -- BASELINE.json config 5 from files in one call.  It is the three
 * per-format batch calls run SIDE BY SIDE, each on a stream of its own behind `stream` and on a worker thread of the library: the
 * PNG leg is bound by the inflate kernels while the QOI leg is bound by PCIe, and the JPEG leg is short.  info[i] receives format
 * and geometry, status_host[i] (may be NULL) the file's status (GAMUT_HIP_ERR_UNSUPPORTED: format not identified).  Returns when
 * the pixels are in place; the status of the lowest-numbered failing file, GAMUT_HIP_OK if none.
 * BMP files (detectBMP, plugins/bmp.d:45-82: 'B', 'M' and a known header size at offset 14; tested after the three signatures above)
 * are a fourth, short leg: gamut_hip_bmp_decode_batch_device on a stream of its own, run from the calling thread once the workers have
 * their legs and before they are waited for.
 * TGA files (detectTGA: gamut_hip_tga_read_header's `detected`; the format has no signature, so it is tested LAST, image.d:1056) are
 * a fifth leg of the same kind, gamut_hip_tga_decode_batch_device, run behind the BMP leg.  A file that is detected and fails to load
 * is that image's GAMUT_HIP_ERR_DECODE. */
enum { GAMUT_HIP_FORMAT_UNKNOWN = -1, GAMUT_HIP_FORMAT_JPEG = 0, GAMUT_HIP_FORMAT_PNG = 1, GAMUT_HIP_FORMAT_QOI = 2, GAMUT_HIP_FORMAT_TGA = 5,
       GAMUT_HIP_FORMAT_BMP = 7 };
typedef struct gamut_hip_image_info { int32_t format, width, height, channels_in_file, channels; } gamut_hip_image_info;
int gamut_hip_identify_format(const uint8_t* data, size_t len);
int gamut_hip_decode_batch_device(const uint8_t* const* data, const size_t* len, int count, int req_comps,
                                  const int64_t* out_offset, uint8_t* out, gamut_hip_image_info* info, int* status_host, void* stream);

/* ---- multi-GPU (north_star: "image-index round-robin, RCCL over xGMI only for the gather of decoded outputs") --
 * One process per GPU.  Images are independent, so the data path has no collective: image i of a batch belongs to rank
 * i % world and is the (i / world)-th image that rank holds.  The reference has no counterpart (single-threaded library);
 * this is what gamut_amd/shard.py does, for a host that is not Python. */
int     gamut_hip_shard_owner(int64_t image_index, int world);                    /* rank that decodes image i */
int64_t gamut_hip_shard_count(int rank, int world, int64_t total_images);         /* images a rank holds */
int64_t gamut_hip_shard_local_index(int64_t image_index, int world);              /* position among its owner's images */
int64_t gamut_hip_shard_global_index(int64_t local_index, int rank, int world);   /* and back */
/* worker threads the host-side feeders start by default: the cores the process may use (cgroup quota) divided by the
 * ranks on this node (LOCAL_WORLD_SIZE / OMPI_COMM_WORLD_LOCAL_SIZE), or GAMUT_HIP_HOST_THREADS */
int     gamut_hip_host_threads(void);

/* The one exchange: gathering decoded outputs.  An RCCL communicator behind an opaque handle; librccl is loaded at run time.
 * Rank 0 calls comm_get_unique_id (128 bytes) and hands the bytes to the other ranks by whatever channel the host has;
 * every rank then calls comm_init with the device it decodes on current (gamut_hip_init).  world == 1 needs no id and no RCCL. */
#define GAMUT_HIP_COMM_ID_BYTES 128
typedef struct gamut_hip_comm gamut_hip_comm;
int  gamut_hip_comm_get_unique_id(void* id128);
int  gamut_hip_comm_init(gamut_hip_comm** comm, int world, int rank, const void* id128);
void gamut_hip_comm_destroy(gamut_hip_comm* comm);
int  gamut_hip_comm_rank(const gamut_hip_comm* comm);
int  gamut_hip_comm_world(const gamut_hip_comm* comm);
/* `local` (HBM): this rank's decoded images, the k-th one at local + k * local_stride, bytes_per_image each.  Image i of
 * the batch arrives at dst + i * dst_stride on `root` (root = -1: on every rank, an all-gather).  Grouped ncclSend /
 * ncclRecv per image on `stream` (asynchronous); a rank's own images are copied device to device.  Collective: every rank
 * of the communicator must call it with the same total_images / bytes_per_image / root. */
int  gamut_hip_gather_outputs_device(gamut_hip_comm* comm, const void* local, int64_t local_stride, int64_t bytes_per_image,
                                     int64_t total_images, void* dst, int64_t dst_stride, int root, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GAMUT_HIP_H */
