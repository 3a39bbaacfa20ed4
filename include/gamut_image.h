/*
 * gamut_image.h -- C ABI of the host-side mirror of Gamut's `Image` for the GPU path.
 *
 * The reference's host API is D (`struct Image`, source/gamut/image.d).  No D compiler exists in the
 * build image, so the same interface is provided in C++ (gamut_amd/csrc/image_host.hip) over the
 * kernels' ABI (gamut_hip.h) and exported here as C functions named after the D members they mirror:
 * same argument meaning, same state machine (error state = static C string + type unknown,
 * image.d:1563-1570), same storage rules (allocatePixelStorage, internals/types.d:355-540), same
 * LoadFlags / LayoutConstraints bits (types.d:139-348).  Pixel storage is host malloc memory exactly as
 * in the reference (the user may disown and free() it); every pixel operation (decode, convertTo) runs
 * on the GPU through gamut_hip_* -- there is no CPU pixel path.
 * Formats read: JPEG (baseline), PNG, QOI, QOIX (the 8-bit colour files), BMP, TGA, SQZ and GIF (every frame a layer of an rgba8
 * image); anything else reports "Unidentified image format".  Formats written: QOI, JPEG and GIF through the generic entries
 * (saveToMemory / saveToFile); PNG, BMP, TGA, QOIX, DDS (written only, never read) and SQZ each through a pair of entries of its own.
 */
#ifndef GAMUT_IMAGE_H
#define GAMUT_IMAGE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* ImageFormat (types.d:14-28) */
enum { GAMUT_FORMAT_unknown = -1, GAMUT_FORMAT_JPEG = 0, GAMUT_FORMAT_PNG = 1, GAMUT_FORMAT_QOI = 2, GAMUT_FORMAT_QOIX = 3, GAMUT_FORMAT_DDS = 4, GAMUT_FORMAT_TGA = 5, GAMUT_FORMAT_GIF = 6, GAMUT_FORMAT_BMP = 7, GAMUT_FORMAT_SQZ = 9 };   /* ImageFormat, types.d:14-21 */

/* LoadFlags (types.d:139-197) */
enum {
    GAMUT_LOAD_NORMAL = 0, GAMUT_LOAD_GREYSCALE = 0x10000, GAMUT_LOAD_ALPHA = 0x20000, GAMUT_LOAD_NO_ALPHA = 0x40000,
    GAMUT_LOAD_RGB = 0x80000, GAMUT_LOAD_8BIT = 0x100000, GAMUT_LOAD_16BIT = 0x200000, GAMUT_LOAD_FP32 = 0x400000,
    GAMUT_LOAD_NO_PIXELS = 0x800000, GAMUT_LOAD_PREMUL = 0x1000000, GAMUT_LOAD_NO_PREMUL = 0x2000000
};
/* LayoutConstraints (types.d:266-348), a ushort */
enum {
    GAMUT_LAYOUT_DEFAULT = 0,
    GAMUT_LAYOUT_MULTIPLICITY_1 = 0, GAMUT_LAYOUT_MULTIPLICITY_2 = 1, GAMUT_LAYOUT_MULTIPLICITY_4 = 2, GAMUT_LAYOUT_MULTIPLICITY_8 = 3,
    GAMUT_LAYOUT_TRAILING_0 = 0, GAMUT_LAYOUT_TRAILING_1 = 4, GAMUT_LAYOUT_TRAILING_3 = 8, GAMUT_LAYOUT_TRAILING_7 = 12,
    GAMUT_LAYOUT_SCANLINE_ALIGNED_1 = 0, GAMUT_LAYOUT_SCANLINE_ALIGNED_2 = 16, GAMUT_LAYOUT_SCANLINE_ALIGNED_4 = 32,
    GAMUT_LAYOUT_SCANLINE_ALIGNED_8 = 48, GAMUT_LAYOUT_SCANLINE_ALIGNED_16 = 64, GAMUT_LAYOUT_SCANLINE_ALIGNED_32 = 80,
    GAMUT_LAYOUT_SCANLINE_ALIGNED_64 = 96, GAMUT_LAYOUT_SCANLINE_ALIGNED_128 = 112,
    GAMUT_LAYOUT_BORDER_0 = 0, GAMUT_LAYOUT_BORDER_1 = 128, GAMUT_LAYOUT_BORDER_2 = 256, GAMUT_LAYOUT_BORDER_3 = 384,
    GAMUT_LAYOUT_VERT_FLIPPED = 512, GAMUT_LAYOUT_VERT_STRAIGHT = 1024, GAMUT_LAYOUT_GAPLESS = 2048
};
/* ops of gamut_convert_pixel_type (types.d:351-602) */
enum { GAMUT_TO_GREYSCALE = 0, GAMUT_TO_RGB, GAMUT_TO_ADD_ALPHA, GAMUT_TO_DROP_ALPHA, GAMUT_TO_PREMUL, GAMUT_TO_NO_PREMUL,
       GAMUT_TO_8BIT, GAMUT_TO_16BIT, GAMUT_TO_FP32 };

typedef struct gamut_image gamut_image;

/* free functions */
int  gamut_convert_pixel_type(int type, int op);                       /* convertPixelTypeTo* */
int  gamut_apply_load_flags(int type, int flags);                      /* internals/types.d:627-661 */
int  gamut_compute_requested_image_components(int flags);              /* internals/types.d:587-609 */
int  gamut_valid_load_flags(int flags);                                /* internals/types.d:563-578 */
int  gamut_layout_constraints_valid(int constraints);                  /* internals/types.d:267-289 */
int  gamut_layout_constraints_compatible(int newer, int older);        /* internals/types.d:241-264 */
int  gamut_identify_format_from_memory(const uint8_t* bytes, size_t len);   /* image.d:1038-1061 (JPEG, PNG, QOI, GIF, BMP; TGA, which has no signature, last) */
void gamut_free_image_data(void* mallocArea);                          /* freeImageData, image.d:27-30 */

/* lifetime: a new image is Image.init = errored with "Uninitialized image" (image.d:1609-1613) */
gamut_image* gamut_image_new(void);
void         gamut_image_delete(gamut_image* img);                     /* ~this: frees owned storage */

/* creation (image.d:565-617, 760-789); return 1 on success like the D members that return bool */
int gamut_image_create(gamut_image* img, int width, int height, int type, int layout);
int gamut_image_create_layered(gamut_image* img, int width, int height, int layers, int type, int layout);
int gamut_image_create_no_init(gamut_image* img, int width, int height, int type, int layout);
int gamut_image_create_layered_no_init(gamut_image* img, int width, int height, int layers, int type, int layout);
int gamut_image_create_with_no_data(gamut_image* img, int width, int height, int type, int layout);
/* createView (image.d:697): borrow caller memory; pitch may be negative */
int gamut_image_create_view(gamut_image* img, void* data, int width, int height, int type, int pitchInBytes);

/* load (image.d:886-906): flags = LOAD_* | LAYOUT_*; returns isValid().  A TGA file (plugins/tga.d:42-95) loads as l8 / la8 / rgb8 /
 * rgba8 by its header, aspect ratio and resolution unknown, then convertTo(applyLoadFlags(type, flags), layout); "Image decoding
 * failed" where the header, the colour map or the pixel stream is refused (gamut_hip_tga_*). */
int gamut_image_load_from_memory(gamut_image* img, const uint8_t* bytes, size_t len, int flags);

/* conversion (image.d:1082-1332): all forward to convertTo */
int gamut_image_convert_to(gamut_image* img, int targetType, int layout);
int gamut_image_set_layout(gamut_image* img, int layout);
int gamut_image_convert_op(gamut_image* img, int op, int layout);      /* convertToGreyscale ... convertToFP32 by GAMUT_TO_* */
int gamut_image_convert_to_greyscale_alpha(gamut_image* img, int layout);
int gamut_image_convert_to_rgba(gamut_image* img, int layout);
int gamut_image_flip_vertical(gamut_image* img);                       /* image.d:1524: the logical flip (pitch negated), or -- when a LAYOUT_VERT_* constraint
                                                                          pins the storage order -- flipVerticalPhysical (:1926-1954), rows swapped on the GPU */
int gamut_image_flip_horizontal(gamut_image* img);                     /* image.d:1475-1509, pixels swapped on the GPU */
/* views and copies (image.d:645-679, 706-752, 795-841).  The returned images are new objects (gamut_image_delete them): a view
 * borrows the pixels (not owned, LAYOUT_DEFAULT), a clone owns its own with the source's layout constraints; both are errored
 * images when the arguments are not what the reference asserts. */
gamut_image* gamut_image_layer_range(gamut_image* img, int layerStart, int layerEnd);     /* layer(i) = layer_range(i, i + 1) */
int gamut_image_create_layered_view(gamut_image* img, void* data, int width, int height, int layers, int type, int pitchInBytes, int layerOffsetBytes);
gamut_image* gamut_image_clone(gamut_image* img);
int gamut_image_copy_pixels_to(gamut_image* img, gamut_image* dst);

/* state (image.d:97-551, 1405-1459) */
int   gamut_image_type(const gamut_image* img);
int   gamut_image_width(const gamut_image* img);
int   gamut_image_height(const gamut_image* img);
int   gamut_image_layers(const gamut_image* img);
int   gamut_image_pitch_in_bytes(const gamut_image* img);
int   gamut_image_layer_offset_in_bytes(const gamut_image* img);
int   gamut_image_scanline_in_bytes(const gamut_image* img);
int   gamut_image_layout_constraints(const gamut_image* img);
int   gamut_image_is_error(const gamut_image* img);
int   gamut_image_is_valid(const gamut_image* img);
const char* gamut_image_error_message(const gamut_image* img);         /* NULL when valid */
int   gamut_image_has_data(const gamut_image* img);
int   gamut_image_is_owned(const gamut_image* img);
int   gamut_image_is_stored_upside_down(const gamut_image* img);
float gamut_image_pixel_aspect_ratio(const gamut_image* img);
float gamut_image_dots_per_inch_y(const gamut_image* img);
uint8_t* gamut_image_scanptr(gamut_image* img, int y);                 /* layer 0 */
uint8_t* gamut_image_layerptr(gamut_image* img, int layer, int y);
uint8_t* gamut_image_disown_data(gamut_image* img);                    /* image.d:483-490 */

/* ---- device-resident pixel storage (an extension: the reference keeps pixels in host memory) --------------------
 * With it on, create*() allocates in HBM, loadFromMemory decodes straight into HBM (JPEG entropy decode included for
 * baseline files) and convertTo / setLayout chains run device to device; scanptr() / layerptr() return DEVICE addresses.
 * Can only be switched while the image owns no pixels; returns 0 otherwise or when there is no GPU. */
int gamut_image_set_device_storage(gamut_image* img, int on);
int gamut_image_is_device(const gamut_image* img);
/* one layer, logical top-down order, into host rows of dst_pitch bytes -- for host and device images alike */
int gamut_image_copy_pixels_to_host(gamut_image* img, int layer, void* dst, int64_t dst_pitch);

/* ---- saving (image.d:940-1011, saveQOI plugins/qoi.d:149-184, saveJPEG plugins/jpeg.d:112-148) ------------------------------
 * Layer 0 in logical top-down order, encoded on the GPU: device-resident images straight from HBM, host images through pinned
 * staging.  QOI (gamut_hip_qoi_encode*): rgb8 / rgba8, colorspace sRGB.  JPEG (gamut_hip_jpeg_encode*, byte for byte what
 * stbi_write_jpg_to_func writes): l8 (one component) / rgb8 (three), quality 90, so 4:2:0; rgba8 and every other type are refused
 * as saveJPEG refuses them.  GIF (gamut_hip_gif_encode*, byte for byte what saveGIF, plugins/gif.d:105-147, writes): rgba8 only, and
 * unlike the other two EVERY layer is encoded, as a frame of 7 centiseconds (any layer count >= 1; upside-down and padded layouts are
 * honoured).  These two generic entries dispatch those three formats only: for GAMUT_FORMAT_PNG, _BMP, _TGA, _QOIX, _DDS and _SQZ
 * they return NULL / 0, as for an errored image or an unknown format, and each of the six is saved through its own
 * gamut_image_save_<format>_to_memory / _to_file pair below.  Flags are ignored here (as the three plugins do; of all the savers
 * only PNG and SQZ read theirs).  The image's state and error are left as they were. */
uint8_t* gamut_image_save_to_memory(gamut_image* img, int fif, int flags, size_t* len);   /* image.d:966-980; NULL (and *len = 0) on refusal */
int      gamut_image_save_to_file(gamut_image* img, int fif, const char* path, int flags); /* image.d:953-958; 1 on success */
void     gamut_free_encoded_image(void* encoded);                                       /* image.d:32-36 */
/* savePNG (plugins/png.d:172-221; gamut_hip_png_*): l8 / la8 / rgb8 / rgba8 / l16 / la16 / rgb16 / rgba16, every other type refused.
 * Unlike the other two plugins this one reads its flags (:201-206, types.d:220-248): level = flags & 15, 0 meaning
 * ENCODE_PNG_COMPRESSION_5, minus 1 (so 12..15 are refused); GAMUT_ENCODE_PNG_FILTER_FAST forces filter 0. */
enum {
    GAMUT_ENCODE_PNG_COMPRESSION_DEFAULT = 0, GAMUT_ENCODE_PNG_COMPRESSION_FAST = 2, GAMUT_ENCODE_PNG_COMPRESSION_SMALL = 10,
    GAMUT_ENCODE_PNG_COMPRESSION_0 = 1, GAMUT_ENCODE_PNG_COMPRESSION_1 = 2, GAMUT_ENCODE_PNG_COMPRESSION_2 = 3,
    GAMUT_ENCODE_PNG_COMPRESSION_3 = 4, GAMUT_ENCODE_PNG_COMPRESSION_4 = 5, GAMUT_ENCODE_PNG_COMPRESSION_5 = 6,
    GAMUT_ENCODE_PNG_COMPRESSION_6 = 7, GAMUT_ENCODE_PNG_COMPRESSION_7 = 8, GAMUT_ENCODE_PNG_COMPRESSION_8 = 9,
    GAMUT_ENCODE_PNG_COMPRESSION_9 = 10, GAMUT_ENCODE_PNG_COMPRESSION_10 = 11,
    GAMUT_ENCODE_PNG_FILTER_DEFAULT = 0, GAMUT_ENCODE_PNG_FILTER_SMALL = 0, GAMUT_ENCODE_PNG_FILTER_FAST = 16
};
uint8_t* gamut_image_save_png_to_memory(gamut_image* img, int flags, size_t* len);      /* NULL (and *len = 0) on refusal */
int      gamut_image_save_png_to_file(gamut_image* img, const char* path, int flags);   /* 1 on success */
/* saveBMP (plugins/bmp.d:166-194; gamut_hip_bmp_*): rgb8 / rgba8 with one layer, 1 <= width, height <= 32767, every other image
 * refused; byte for byte write_bmp (bmpenc.d), with biX/YPelsPerMeter = round(pixelsPerMeterX / Y) or 0 when unknown; flags are
 * ignored as saveBMP ignores them.  The image's state and error are left as they were.  Freed with gamut_free_encoded_image. */
uint8_t* gamut_image_save_bmp_to_memory(gamut_image* img, int flags, size_t* len);      /* NULL (and *len = 0) on refusal */
int      gamut_image_save_bmp_to_file(gamut_image* img, const char* path, int flags);   /* 1 on success */
/* saveTGA (plugins/tga.d:128-150; gamut_hip_tga_encode*): l8 / la8 / rgb8 / rgba8, every other type refused as TGAEncoder.initialize
 * refuses it; layer 0 of a layered image (saveTGA walks scanptr(y)); always run-length encoded, flags are ignored; 1 <= width, height
 * <= 65535.  GAMUT_FORMAT_TGA (5) is not dispatched from the two generic entries above (they return NULL / 0 for it).  The image's
 * state and error are left as they were.  Freed with gamut_free_encoded_image. */
uint8_t* gamut_image_save_tga_to_memory(gamut_image* img, int flags, size_t* len);      /* NULL (and *len = 0) on refusal */
int      gamut_image_save_tga_to_file(gamut_image* img, const char* path, int flags);   /* 1 on success */
/* saveQOIX (plugins/qoix.d:156-242; gamut_hip_qoix_encode*), the 8-bit colour slice: rgb8 (3 channels, colorspace 0), rgba8 (4, 0) and
 * rgbap8 (4, colorspace 2); every other type is refused -- the grey and 16-bit types until their codecs exist on both sides.  Layer 0
 * of a layered image; pixelAspectRatio and dotsPerInchY go into the header bit for bit; LZ4 when that file is smaller; flags are
 * ignored.  GAMUT_FORMAT_QOIX (3) is not dispatched from the two generic entries above (they return NULL / 0 for it).  The image's
 * state and error are left as they were.  Freed with gamut_free_encoded_image. */
uint8_t* gamut_image_save_qoix_to_memory(gamut_image* img, int flags, size_t* len);     /* NULL (and *len = 0) on refusal */
int      gamut_image_save_qoix_to_file(gamut_image* img, const char* path, int flags);  /* 1 on success */
/* saveDDS (plugins/dds.d:47-216; gamut_hip_dds_encode*): l8 / la8 / rgb8 / rgba8 as BC7 blocks behind a DX10 header; every other type
 * is refused, lap8 and rgbap8 included (saveDDS's switch has no case for them).  Layer 0 of a layered image; flags are ignored.
 * GAMUT_FORMAT_DDS (4) is not dispatched from the two generic entries above (they return NULL / 0 for it), and no DDS file is
 * identified or loaded, as in the reference.  The image's state and error are left as they were.  Freed with gamut_free_encoded_image. */
uint8_t* gamut_image_save_dds_to_memory(gamut_image* img, int flags, size_t* len);      /* NULL (and *len = 0) on refusal */
int      gamut_image_save_dds_to_file(gamut_image* img, const char* path, int flags);   /* 1 on success */
/* saveSQZ (plugins/sqz.d:141-201; gamut_hip_sqz_encode*): rgb8 only, both sides at least 8, layer 0 of a layered image; Oklab, 7
 * levels (clamped to what the size admits), chroma scheduled one round later, snake scan.  The flags carry the byte budget
 * (GAMUT_ENCODE_SQZ_QUALITY_*, gamut_hip_sqz_budget_from_flags); the file is the bytes the stream used, which is less than the budget
 * when the image is lossless below it.  GAMUT_FORMAT_SQZ (9) is not dispatched from the two generic entries above (they return
 * NULL / 0 for it).  Host-resident and device-resident images; the image's state and error are left as they were.  Freed with
 * gamut_free_encoded_image. */
enum {
    GAMUT_ENCODE_SQZ_QUALITY_DEFAULT = 0,          /* 2.5 bits per pixel */
    GAMUT_ENCODE_SQZ_QUALITY_BPP1_0 = 0x20 << 5, GAMUT_ENCODE_SQZ_QUALITY_BPP1_25 = 0x28 << 5, GAMUT_ENCODE_SQZ_QUALITY_BPP1_5 = 0x30 << 5,
    GAMUT_ENCODE_SQZ_QUALITY_BPP1_75 = 0x38 << 5, GAMUT_ENCODE_SQZ_QUALITY_BPP2_0 = 0x40 << 5, GAMUT_ENCODE_SQZ_QUALITY_BPP2_25 = 0x48 << 5,
    GAMUT_ENCODE_SQZ_QUALITY_BPP2_5 = 0x50 << 5, GAMUT_ENCODE_SQZ_QUALITY_BPP2_75 = 0x58 << 5, GAMUT_ENCODE_SQZ_QUALITY_BPP3_0 = 0x60 << 5,
    GAMUT_ENCODE_SQZ_QUALITY_BPP3_25 = 0x68 << 5, GAMUT_ENCODE_SQZ_QUALITY_BPP3_5 = 0x70 << 5, GAMUT_ENCODE_SQZ_QUALITY_BPP3_75 = 0x78 << 5,
    GAMUT_ENCODE_SQZ_QUALITY_MAX = 0xff << 5       /* about 8 bits per pixel */
};
uint8_t* gamut_image_save_sqz_to_memory(gamut_image* img, int flags, size_t* len);      /* NULL (and *len = 0) on refusal */
int      gamut_image_save_sqz_to_file(gamut_image* img, const char* path, int flags);   /* 1 on success */
/* The two above run the writer gamut_hip_sqz_set_writer names (GAMUT_HIP_SQZ_WRITER); the files are the same bytes either way.
 * saveSQZ of a DEVICE-resident rgb8 image with the file left in HBM (always the device writer; no coefficient and no file byte
 * crosses the bus): the DEVICE address of the file and *len, or NULL (and *len = 0) on refusal -- a host-resident image included.
 * Ownership is that of the image's device pixel storage: the buffer belongs to the image, stays valid until the next
 * gamut_image_save_sqz_to_device on this image or gamut_image_delete, and is never freed by the caller. */
uint8_t* gamut_image_save_sqz_to_device(gamut_image* img, int flags, size_t* len);

#ifdef __cplusplus
}
#endif
#endif
