// image_host.hip -- host-side mirror of Gamut's `struct Image` (source/gamut/image.d) for the GPU path,
// exported through include/gamut_image.h.  Written in C++ because the image has no D compiler; member
// names, state and error strings follow the reference so a test written against image.d reads the same.
//
//   fields                       image.d:1573-1620
//   error state                  image.d:1563-1570, internals/errors.d:14-35
//   allocatePixelStorage         internals/types.d:355-540      (border / trailing / multiplicity / alignment / v-flip / bonus bytes)
//   layout constraint helpers    internals/types.d:166-289
//   load flags                   internals/types.d:563-661, types.d:351-602
// Optionally the storage is device memory (gamut_image_set_device_storage): decode and convertTo chains then never leave HBM.
//   loadFromMemory               image.d:886-901, 1751-1772 ; loadJPEG plugins/jpeg.d:42-104 ; loadPNG plugins/png.d:44-163 ;
//                                loadQOI plugins/qoi.d:47-141
//   convertTo                    image.d:1180-1332 ; getAdHocLayoutConstraints :1809-1905
//
// Pixel storage is host malloc memory, as in the reference.  Every pixel operation goes to the GPU through
// the C ABI of gamut_hip.h (host drop-ins); nothing is computed on the CPU here.
#include "encode_host.hpp"
#include "../../include/gamut_image.h"
#include <new>

namespace {

using namespace gamut;

const char* const kStrImageHasNoType           = "Image has no type";
const char* const kStrImageDecodingFailed      = "Image decoding failed";
const char* const kStrImageDecodingIOFailure   = "I/O failure while decoding image";
const char* const kStrImageFormatUnidentified  = "Unidentified image format";
const char* const kStrImageNotInitialized      = "Uninitialized image";
const char* const kStrImageTooLarge            = "Can't have an image that exceeds Gamut size limitations";
const char* const kStrImageWrongComponents     = "Invalid number of component for image";
const char* const kStrInvalidFlags             = "Invalid image decoding flags";
const char* const kStrIllegalNegativeDimension = "Illegal negative dimension";
const char* const kStrIllegalLayoutConstraints = "Cannot satisfy illegal layout constraints";
const char* const kStrOutOfMemory              = "Out of memory";
const char* const kStrUnsupportedTypeConversion= "Unsupported image pixel type conversion";
const char* const kStrUnsupportedVFlip __attribute__((unused)) = "Can't flip image vertically";   // (flipVerticalLogical under a VERT constraint: not reachable through flipVertical, which goes physical then)
const char* const kStrOverlappingScanlines     = "Scanlines are overlapping";
const char* const kStrOverlappingLayers        = "Layers are overlapping";
const char* const kStrInvalidNegLayerOffset    = "Invalid negative layer offset";

constexpr int  MAX_W = 16777216, MAX_H = 16777216, MAX_LAYERS = 4194303;          // types.d:103-110
constexpr long long MAX_BYTES = 34359738368LL;                                     // types.d:117
constexpr int  BORDER_MASK = 384;
constexpr float kInchesPerMeter = 39.37007874f;                                    // convertInchesToMeters / convertMetersToInches (types.d:126-135)
// components -> the 8-bit / 16-bit PixelType a decoder hands back
constexpr int kType8[5]  = { -1, GAMUT_PIXEL_l8, GAMUT_PIXEL_la8, GAMUT_PIXEL_rgb8, GAMUT_PIXEL_rgba8 };
constexpr int kType16[5] = { -1, GAMUT_PIXEL_l16, GAMUT_PIXEL_la16, GAMUT_PIXEL_rgb16, GAMUT_PIXEL_rgba16 };

// ---- layout constraint helpers (internals/types.d:166-289) ----
int layoutMultiplicity(int c)      { return 1 << (c & 3); }
int layoutTrailingPixels(int c)    { return (1 << ((c & 0x0C) >> 2)) - 1; }
int layoutScanlineAlignment(int c) { return 1 << ((c >> 4) & 0x0f); }
int layoutBorderWidth(int c)       { return (c >> 7) & 3; }
bool layoutGapless(int c)          { return (c & GAMUT_LAYOUT_GAPLESS) != 0; }

bool layoutConstraintsValid(int c)
{
    if ((c & GAMUT_LAYOUT_VERT_FLIPPED) && (c & GAMUT_LAYOUT_VERT_STRAIGHT)) return false;
    if (layoutGapless(c)) {
        if (layoutMultiplicity(c) > 1 || layoutTrailingPixels(c) > 0 || layoutScanlineAlignment(c) > 1 || layoutBorderWidth(c) > 0) return false;
    }
    return true;
}
bool layoutConstraintsCompatible(int newer, int older)
{
    if ((newer & GAMUT_LAYOUT_GAPLESS) && !(older & GAMUT_LAYOUT_GAPLESS)) return false;
    if ((newer & GAMUT_LAYOUT_VERT_FLIPPED) && !(older & GAMUT_LAYOUT_VERT_FLIPPED)) return false;
    if ((newer & GAMUT_LAYOUT_VERT_STRAIGHT) && !(older & GAMUT_LAYOUT_VERT_STRAIGHT)) return false;
    if (layoutMultiplicity(newer) > layoutMultiplicity(older)) return false;
    if (layoutTrailingPixels(newer) > layoutTrailingPixels(older)) return false;
    if (layoutScanlineAlignment(newer) > layoutScanlineAlignment(older)) return false;
    if (layoutBorderWidth(newer) > layoutBorderWidth(older)) return false;
    return true;
}
int pointerAlignment(size_t p)      // getPointerAlignment, internals/types.d:202-213
{
    for (int k = 7; k >= 1; --k) if ((p & ((size_t(1) << k) - 1)) == 0) return k << 4;
    return 0;
}
bool imageIsValidSize(int layers, int w, int h)
{
    return !(layers < 0 || w < 0 || h < 0 || layers > MAX_LAYERS || w > MAX_W || h > MAX_H);
}

// ---- PixelType algebra (types.d:351-602): type = family*3 + depth, family l, la, lap, rgb, rgba, rgbap ----
int convertPixelType(int t, int op)
{
    if (!valid_type(t)) return GAMUT_PIXEL_unknown;
    int fam = t / 3, depth = t % 3;
    switch (op) {
    case GAMUT_TO_GREYSCALE:  if (fam >= 3) fam -= 3; break;
    case GAMUT_TO_RGB:        if (fam < 3) fam += 3; break;
    case GAMUT_TO_ADD_ALPHA:  if (fam == 0 || fam == 3) fam += 1; break;
    case GAMUT_TO_DROP_ALPHA: if (fam == 1 || fam == 2) fam = 0; else if (fam >= 4) fam = 3; break;
    case GAMUT_TO_PREMUL:     if (fam == 1 || fam == 4) fam += 1; break;
    case GAMUT_TO_NO_PREMUL:  if (fam == 2 || fam == 5) fam -= 1; break;
    case GAMUT_TO_8BIT:  depth = 0; break;
    case GAMUT_TO_16BIT: depth = 1; break;
    case GAMUT_TO_FP32:  depth = 2; break;
    default: return GAMUT_PIXEL_unknown;
    }
    return fam * 3 + depth;
}
bool validLoadFlags(int f)          // internals/types.d:563-578
{
    if ((f & GAMUT_LOAD_GREYSCALE) && (f & GAMUT_LOAD_RGB)) return false;
    if ((f & GAMUT_LOAD_ALPHA) && (f & GAMUT_LOAD_NO_ALPHA)) return false;
    if ((f & GAMUT_LOAD_PREMUL) && (f & GAMUT_LOAD_NO_PREMUL)) return false;
    int bits = 0;
    if (f & GAMUT_LOAD_8BIT) ++bits;
    if (f & GAMUT_LOAD_16BIT) ++bits;
    if (f & GAMUT_LOAD_FP32) ++bits;
    return bits <= 1;
}
int computeRequestedImageComponents(int f)      // internals/types.d:587-609
{
    int req = -1;
    if (!validLoadFlags(f)) return 0;
    if (f & GAMUT_LOAD_GREYSCALE) { if (f & GAMUT_LOAD_ALPHA) req = 2; else if (f & GAMUT_LOAD_NO_ALPHA) req = 1; }
    else if (f & GAMUT_LOAD_RGB)  { if (f & GAMUT_LOAD_ALPHA) req = 4; else if (f & GAMUT_LOAD_NO_ALPHA) req = 3; }
    return req;
}
int applyLoadFlags(int type, int f)             // internals/types.d:627-661
{
    if (!validLoadFlags(f)) return GAMUT_PIXEL_unknown;
    static const int order[][2] = { { GAMUT_LOAD_GREYSCALE, GAMUT_TO_GREYSCALE }, { GAMUT_LOAD_RGB, GAMUT_TO_RGB },
        { GAMUT_LOAD_ALPHA, GAMUT_TO_ADD_ALPHA }, { GAMUT_LOAD_NO_ALPHA, GAMUT_TO_DROP_ALPHA }, { GAMUT_LOAD_8BIT, GAMUT_TO_8BIT },
        { GAMUT_LOAD_16BIT, GAMUT_TO_16BIT }, { GAMUT_LOAD_FP32, GAMUT_TO_FP32 }, { GAMUT_LOAD_PREMUL, GAMUT_TO_PREMUL },
        { GAMUT_LOAD_NO_PREMUL, GAMUT_TO_NO_PREMUL } };
    for (auto& o : order) if (f & o[0]) type = convertPixelType(type, o[1]);
    return type;
}

// ---- pixel storage (what internals/types.d:355-540 allocates, and where the first pixel stands in it) ----
// The layout constraints translate into a geometry -- bytes per row, rows per layer, the byte where pixel (0, 0) of layer 0 stands -- that is
// worked out first and on its own (PlaneGeometry::plan), the same for host and HBM storage; getting the bytes and orienting the rows come after.
struct Storage { uint8_t* data = nullptr; uint8_t* alloc = nullptr; int pitch = 0; int layerOffset = 0; };
struct PlaneGeometry {
    int row_bytes = 0;            // distance between two rows (before any flip), a multiple of the scanline alignment
    long long layer_rows = 0;     // rows one layer occupies, its borders included
    long long total = 0;          // bytes to obtain: all layers + slack to align the first row + the caller's bonus bytes in front
    size_t lead = 0;              // bytes in front of pixel (0, 0) of layer 0 (bonus bytes, the top border's rows, the left border) before alignment
    int align = 1;
    static size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }
    bool plan(int type, int layers, int w, int h, int constraints, int bonus)
    {
        const int frame = layoutBorderWidth(constraints);                       // pixels around every layer
        const int tail = layoutTrailingPixels(constraints), step = layoutMultiplicity(constraints);
        align = layoutScanlineAlignment(constraints);
        const int px = kPixelSize[type];
        // behind the last pixel of a row: the frame, widened until (left frame + width) is a whole number of `step` pixels, and never
        // fewer than the trailing pixels the constraint asks for
        const int used = frame + w;
        const int right = std::max(tail, frame + (int)(round_up((size_t)used, (size_t)step) - (size_t)used));
        row_bytes = (int)round_up((size_t)px * (size_t)(used + right), (size_t)align);
        layer_rows = (long long)h + 2LL * frame;
        total = (long long)row_bytes * layer_rows * layers + (align - 1) + bonus;
        lead = (size_t)bonus + (size_t)row_bytes * (size_t)frame + (size_t)px * (size_t)frame;
        return total <= MAX_BYTES;
    }
};
// device: the pixels live in HBM (hipMalloc) instead of host malloc memory -- same geometry on the device address
bool allocatePixelStorage(uint8_t* existing, int type, int layers, int width, int height, int constraints, int bonusBytes,
                          bool clearWithZeroes, Storage& out, bool device = false)
{
    if (!imageIsValidSize(layers, width, height)) return false;
    PlaneGeometry g;
    if (!g.plan(type, layers, width, height, constraints, bonusBytes)) return false;
    const size_t bytes = (size_t)g.total;
    uint8_t* base = nullptr;
    auto give_back = [&] { if (device) (void)hipFree(base); else free(base); };
    if (device) {
        if (existing) (void)hipFree(existing);
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return false;
        base = (uint8_t*)p;
        if (clearWithZeroes && bytes && hipMemset(base, 0, bytes) != hipSuccess) { give_back(); return false; }
    } else {
        base = (uint8_t*)realloc(existing, bytes);
        if (bytes && !base) return false;
        if (clearWithZeroes && bytes) memset(base, 0, bytes);
    }
    const long long between_layers = layers > 1 ? (long long)g.row_bytes * g.layer_rows : 0;
    if (between_layers > 2147483647LL) { give_back(); return false; }
    uint8_t* origin = (uint8_t*)PlaneGeometry::round_up((size_t)(base + g.lead), (size_t)g.align);
    // rows stored bottom-up when the constraint says so (flipScanlinePointers :294-306: the pointer goes to the last row, the pitch turns negative)
    const bool bottom_up = (constraints & GAMUT_LAYOUT_VERT_FLIPPED) != 0;
    out.alloc = base;
    out.data = bottom_up && height >= 2 ? origin + (ptrdiff_t)g.row_bytes * (height - 1) : origin;
    out.pitch = bottom_up ? -g.row_bytes : g.row_bytes;
    out.layerOffset = (int)between_layers;
    return true;
}

} // namespace

// fields in the reference's declaration order (image.d:1573-1620)
struct gamut_image {
    int       _type = GAMUT_PIXEL_unknown;
    uint16_t  _layoutConstraints = 0;
    uint8_t*  _data = nullptr;
    uint8_t*  _allocArea = nullptr;
    int       _width = 0, _height = 0, _layerCount = 0;
    int       _pitch = 0, _layerOffset = 0;
    const char* _error = kStrImageNotInitialized;
    float     _pixelAspectRatio = -1, _resolutionY = -1;
    // Not in the reference: where the pixel storage lives.  false = host malloc memory (the reference's model: every
    // convertTo crosses PCIe twice); true = HBM (hipMalloc): loadFromMemory decodes straight into it and convertTo chains stay
    // on the device; _data / scanptr() are then device addresses (gamut_image_copy_pixels_to_host reads them back).
    bool      _device = false;
    // Not in the reference either: the file gamut_image_save_sqz_to_device left in HBM.  Owned by the image like its device pixel
    // storage: freed by the next such save and by gamut_image_delete.
    uint8_t*  _deviceFile = nullptr;

    void error(const char* msg) { _error = msg; _type = GAMUT_PIXEL_unknown; }           // image.d:1563-1570
    void clearError() { _error = nullptr; }
    bool isValid() const { return _error == nullptr; }
    bool hasData() const { return _data != nullptr; }
    void release(uint8_t* p) const { if (!p) return; if (_device) (void)hipFree(p); else free(p); }
    void cleanupBitmapIfOwned() { if (_allocArea) { release(_allocArea); _allocArea = nullptr; _data = nullptr; } }
    void cleanupBitmapAndTypeIfAny() { cleanupBitmapIfOwned(); _data = nullptr; _type = GAMUT_PIXEL_unknown; _error = kStrImageHasNoType; }

    bool forgetPreviousUsage(int layers, int w, int h)                                     // image.d:1624-1645
    {
        cleanupBitmapAndTypeIfAny();
        clearError();
        if (layers < 0 || w < 0 || h < 0) { error(kStrIllegalNegativeDimension); return false; }
        if (!imageIsValidSize(layers, w, h)) { error(kStrImageTooLarge); return false; }
        return true;
    }
    bool setStorage(int w, int h, int layers, int type, int constraints, bool clear)       // image.d:1677-1727
    {
        if (!valid_type(type)) { error(kStrUnsupportedTypeConversion); return false; }
        if (!layoutConstraintsValid(constraints)) { error(kStrIllegalLayoutConstraints); return false; }
        Storage s;
        if (!allocatePixelStorage(_allocArea, type, layers, w, h, constraints, 0, clear, s, _device)) { _allocArea = nullptr; error(kStrOutOfMemory); return false; }
        _data = s.data; _allocArea = s.alloc; _type = type; _width = w; _height = h; _pitch = s.pitch;
        _layoutConstraints = (uint16_t)constraints; _layerCount = layers; _layerOffset = s.layerOffset;
        return true;
    }
    bool createLayered(int w, int h, int layers, int type, int constraints, bool clear)
    {
        if (!forgetPreviousUsage(layers, w, h)) return false;
        return setStorage(w, h, layers, type, constraints, clear);
    }

    // What the storage AS IT STANDS would satisfy (Image.getAdHocLayoutConstraints, image.d:1809-1905), field by field of the constraint
    // word.  The two power-of-two fields are logarithms: MULTIPLICITY_n = log2 n in bits 0-1, TRAILING_(n-1) = log2 n in bits 2-3, so both
    // come from one question -- how many whole pixels fit between the end of a row and the start of the next -- asked once.
    int getAdHocLayoutConstraints() const
    {
        const auto log2_upto8 = [](int n) { return n >= 8 ? 3 : n >= 4 ? 2 : n >= 2 ? 1 : 0; };
        const int step = _pitch < 0 ? -_pitch : _pitch;                                      // bytes from a row to its neighbour in memory
        const int px = kPixelSize[_type];
        const int spare = log2_upto8((step - _width * px) / px + 1);                         // 1 / 3 / 7 pixels to spare behind a row: rows of 2 / 4 / 8
        const int width_pow = _width % 8 == 0 ? 3 : _width % 4 == 0 ? 2 : _width % 2 == 0 ? 1 : 0;   // the width itself a multiple
        const int promised = _layoutConstraints & 3;                                         // what the image was allocated under still holds
        int word = std::max(promised, std::max(spare, width_pow))                            // multiplicity: any of the three witnesses
                 | spare << 2                                                                // trailing pixels: only what is there
                 | std::min(pointerAlignment((size_t)_data), pointerAlignment((size_t)step)) // every row as aligned as the first one and the step
                 | (_layoutConstraints & BORDER_MASK);                                       // a border cannot be seen in the numbers: the promise
        if (_pitch >= 0) word |= GAMUT_LAYOUT_VERT_STRAIGHT;                                 // (a pitch of 0 -- one row, or none -- is both)
        if (_pitch <= 0) word |= GAMUT_LAYOUT_VERT_FLIPPED;
        const bool layers_abut = _layerCount <= 1 || _layerOffset == step * _height;
        if (_pitch >= 0 && layers_abut) word |= GAMUT_LAYOUT_GAPLESS;                        // the reference asks no more of the rows than pitch == |pitch| (:1886)
        return word;
    }

    bool convertTo(int targetType, int layoutConstraints)                                  // image.d:1180-1332
    {
        if (!isValid()) return false;
        layoutConstraints &= 0xFFFF;
        if (!valid_type(targetType)) { error(kStrUnsupportedTypeConversion); return false; }
        if (!layoutConstraintsValid(layoutConstraints)) { error(kStrIllegalLayoutConstraints); return false; }
        if (!hasData()) { _type = targetType; _layoutConstraints = (uint16_t)layoutConstraints; return true; }
        const bool compatible = layoutConstraintsCompatible(layoutConstraints, getAdHocLayoutConstraints());
        if (_type == targetType && compatible) { _layoutConstraints = (uint16_t)layoutConstraints; return true; }
        if ((_width == 0 || _height == 0 || _layerCount == 0) && compatible) { _layoutConstraints = (uint16_t)layoutConstraints; return true; }

        const int interType = gamut_hip_scanlines_inter_type(_type, targetType);
        const int bonusBytes = targetType != _type ? _width * kPixelSize[interType] : 0;      // the scratch row the reference reserves (:1238-1241)
        Storage s;
        if (!allocatePixelStorage(nullptr, targetType, _layerCount, _width, _height, layoutConstraints, bonusBytes, false, s, _device)) {
            error(kStrOutOfMemory); return false;
        }
        bool ok = true;
        if (_device) {                                                                        // all layers in one launch, nothing leaves HBM
            ok = gamut_hip_scanlines_convert_device(_type, _data, _pitch, _layerOffset, targetType, s.data, s.pitch, s.layerOffset,
                                                    _width, _height, _layerCount, nullptr) == GAMUT_HIP_OK &&
                 gamut_hip_stream_synchronize(nullptr) == GAMUT_HIP_OK;
        } else {
            const uint8_t* srcLayer = _data; uint8_t* dstLayer = s.data;
            for (int layer = 0; layer < _layerCount && ok; ++layer) {                         // :1273-1311, one GPU pass per layer
                ok = gamut_hip_scanlines_convert(_type, srcLayer, _pitch, targetType, dstLayer, s.pitch, _width, _height) == GAMUT_HIP_OK;
                srcLayer += _layerOffset; dstLayer += s.layerOffset;
            }
        }
        if (!ok) { release(s.alloc); error(kStrUnsupportedTypeConversion); return false; }   // keeps the former pixels (:1313-1319)
        const int layers = _layerCount, w = _width, h = _height;
        cleanupBitmapIfOwned();
        _layoutConstraints = (uint16_t)layoutConstraints; _data = s.data; _allocArea = s.alloc; _type = targetType;
        _pitch = s.pitch; _layerCount = layers; _layerOffset = s.layerOffset; _width = w; _height = h; _error = nullptr;
        return true;
    }

    void adopt(uint8_t* decoded, int w, int h, int type, int comps_bytes, float aspect, float resY)   // jpeg.d:82-100 / png.d:108-157
    {
        _type = type; _width = w; _height = h; _allocArea = decoded; _data = decoded; _pitch = w * comps_bytes;
        _pixelAspectRatio = aspect; _resolutionY = resY; _layoutConstraints = GAMUT_LAYOUT_DEFAULT; _layerCount = 1; _layerOffset = 0;
    }

    static uint8_t* dmalloc(size_t n) { void* p = nullptr; return hipMalloc(&p, n ? n : 1) == hipSuccess ? (uint8_t*)p : nullptr; }
    // ONE image through a codec's batch entry: nbytes of HBM and decode(dev, &zero, &status), the entry on a batch of one at offset 0.
    // The pixels stay in HBM; NULL, and nothing left to free, when the allocation or the decode fails.
    template <class Decode> static uint8_t* decodeOneToDevice(size_t nbytes, Decode decode)
    {
        uint8_t* dev = dmalloc(nbytes);
        const int64_t zero = 0; int status = 0;
        if (dev && decode(dev, &zero, &status) != GAMUT_HIP_OK) { (void)hipFree(dev); dev = nullptr; }
        return dev;
    }
    // The same with the pixels handed over where the image keeps them.  The decode is the GPU's either way: a device image keeps the
    // allocation (its rows are tight), a host image gets a malloc'd copy and the allocation is freed.  NULL when any step fails.
    template <class Decode> uint8_t* decodeOne(size_t nbytes, Decode decode) const
    {
        uint8_t* dev = decodeOneToDevice(nbytes, decode);
        if (_device || !dev) return dev;
        uint8_t* host = (uint8_t*)malloc(nbytes ? nbytes : 1);
        const bool ok = host && gamut_hip_memcpy_d2h(host, dev, nbytes, nullptr) == GAMUT_HIP_OK && gamut_hip_stream_synchronize(nullptr) == GAMUT_HIP_OK;
        (void)hipFree(dev);
        if (!ok) { free(host); host = nullptr; }
        return host;
    }

    // decompress_jpeg_image_from_stream with the result left in HBM: host feeder + coefficient upload, then the reconstruction kernels
    uint8_t* decodeJpegToDevice(const uint8_t* bytes, size_t len, int* w, int* h, int* actual, float* aspect, float* dpiY, int req)
    {
        if (req != -1 && req != 1 && req != 3 && req != 4) return nullptr;
        gamut_hip_jpeg_frame f;
        if (gamut_hip_jpeg_read_header(bytes, len, &f) != GAMUT_HIP_OK) return nullptr;
        const size_t nblk = (size_t)f.mcus_per_row * f.mcus_per_col * f.blocks_per_mcu;
        const int comps = req < 0 ? f.comps : req;
        // the coefficient staging is per-thread and stays (only the pixels, which become the image's storage, are a fresh allocation)
        static thread_local PerDevice<DeviceScratch> s_co_pd, s_zz_pd;
        DeviceScratch& s_co = s_co_pd.cur(); DeviceScratch& s_zz = s_zz_pd.cur();
        uint8_t* dco = (uint8_t*)s_co.get(nblk * 128 + 16), *dzz = (uint8_t*)s_zz.get(nblk + 16), *dout = dmalloc((size_t)f.width * f.height * comps);
        bool ok = dco && dzz && dout;
        if (ok) {
            // ONE image: the host feeder (one thread, 1-8 ms for a 1080p file) and an upload of its coefficients.  The device
            // entropy decoders are batch machinery -- a long scan costs their workgroup ~4 ms whatever else the chip does, and
            // the call's staging, threads and events another ~0.5 ms (640 x 480: 0.86 ms against 0.43 this way).
            gamut_hip_jpeg_frame hf;
            int rc = gamut_hip_jpeg_decode_coeffs(bytes, len, &hf);
            if (rc == GAMUT_HIP_OK) {
                rc = gamut_hip_memcpy_h2d(dco, hf.coeffs, nblk * 128, nullptr) | gamut_hip_memcpy_h2d(dzz, hf.max_zag, nblk, nullptr) |
                     gamut_hip_stream_synchronize(nullptr);
                f.pixel_aspect_ratio = hf.pixel_aspect_ratio; f.dpi_y = hf.dpi_y;      // a JFIF / EXIF segment behind the scan counts too (find_eoi, jpegload.d:2826-2848)
                gamut_hip_jpeg_frame_free(&hf);
            }
            ok = rc == GAMUT_HIP_OK &&
                 gamut_hip_jpeg_reconstruct_batch_device((const int16_t*)dco, 0, dzz, 0, dout, (int64_t)f.width * comps, 0, f.width, f.height,
                                                         f.scan_type, comps, 1, nullptr) == GAMUT_HIP_OK &&
                 gamut_hip_stream_synchronize(nullptr) == GAMUT_HIP_OK;
        }
        if (!ok) { if (dout) (void)hipFree(dout); return nullptr; }
        *w = f.width; *h = f.height; *actual = f.comps; *aspect = f.pixel_aspect_ratio; *dpiY = f.dpi_y;
        return dout;
    }

    void loadJPEG(const uint8_t* bytes, size_t len, int flags)                              // plugins/jpeg.d:42-104
    {
        int requested = computeRequestedImageComponents(flags);
        if (requested == 0) { error(kStrInvalidFlags); return; }
        if (requested == 2) requested = -1;
        int w = 0, h = 0, actual = 0; float aspect = -1, dpiY = -1;
        uint8_t* decoded = _device ? decodeJpegToDevice(bytes, len, &w, &h, &actual, &aspect, &dpiY, requested)
                                   : gamut_hip_decompress_jpeg_image_from_memory(bytes, len, &w, &h, &actual, &aspect, &dpiY, requested);
        if (!decoded) { error(kStrImageDecodingFailed); return; }
        if (actual != 1 && actual != 3 && actual != 4) { error(kStrImageWrongComponents); release(decoded); return; }
        if (!imageIsValidSize(1, w, h)) { error(kStrImageTooLarge); release(decoded); return; }
        const int comps = requested == -1 ? actual : requested;
        adopt(decoded, w, h, comps == 1 ? GAMUT_PIXEL_l8 : comps == 3 ? GAMUT_PIXEL_rgb8 : GAMUT_PIXEL_rgba8, comps, aspect, dpiY);
        convertTo(applyLoadFlags(_type, flags), flags & 0xFFFF);
    }
    void loadPNG(const uint8_t* bytes, size_t len, int flags)                               // plugins/png.d:44-163
    {
        const bool is16 = gamut_hip_png_is16(bytes, len) != 0;
        int requested = computeRequestedImageComponents(flags);
        if (requested == 0) { error(kStrInvalidFlags); return; }
        if (requested == -1) requested = 0;
        bool to16 = is16;
        if (flags & GAMUT_LOAD_8BIT) to16 = false;
        if (flags & GAMUT_LOAD_16BIT) to16 = true;
        int w = 0, h = 0, comps = 0; float ppmX = -1, ppmY = -1, ratio = -1;
        uint8_t* decoded = nullptr;
        if (_device) {                                                                      // stbi_load(_16) with the result left in HBM
            gamut_hip_png_info hd, info;
            if (gamut_hip_png_read_header(bytes, len, &hd) == GAMUT_HIP_OK)
                decoded = decodeOneToDevice((size_t)hd.width * hd.height * 4 * (to16 ? 2 : 1) + 64,    // room for any channel count
                                            [&](uint8_t* dev, const int64_t* zero, int* st) {
                    return gamut_hip_png_decode_batch_device(&bytes, &len, 1, requested, to16 ? 16 : 8, zero, dev, &info, st, 1, nullptr);
                });
            if (decoded) {
                w = (int)info.width; h = (int)info.height; comps = info.channels_in_file;
                ppmX = info.pixels_per_meter_x; ppmY = info.pixels_per_meter_y; ratio = info.pixel_aspect_ratio;
            }
        } else {
            decoded = to16 ? (uint8_t*)gamut_hip_stbi_load_16_from_memory(bytes, len, &w, &h, &comps, requested, &ppmX, &ppmY, &ratio)
                           : gamut_hip_stbi_load_from_memory(bytes, len, &w, &h, &comps, requested, &ppmX, &ppmY, &ratio);
        }
        if (requested != 0) comps = requested;
        if (!decoded) { error(kStrImageDecodingFailed); return; }
        if (!imageIsValidSize(1, w, h)) { error(kStrImageTooLarge); release(decoded); return; }
        adopt(decoded, w, h, (to16 ? kType16 : kType8)[comps], comps * (to16 ? 2 : 1), ratio == -1 ? -1.0f : ratio,
              ppmY == -1 ? -1.0f : ppmY / kInchesPerMeter);
        convertTo(applyLoadFlags(_type, flags), flags & 0xFFFF);
    }
    void loadQOI(const uint8_t* bytes, size_t len, int flags)                               // plugins/qoi.d:47-141
    {
        int requested = computeRequestedImageComponents(flags);
        if (requested == 0) { error(kStrInvalidFlags); return; }
        if (requested == -1 || requested == 1 || requested == 2) requested = 0;             // the QOI decoder only makes RGB / RGBA (:81-83)
        gamut_hip_qoi_desc desc;
        uint8_t* decoded = nullptr;
        if (_device) {
            const int size = (int)len;
            if (gamut_hip_qoi_read_header(bytes, size, &desc) == GAMUT_HIP_OK)
                decoded = decodeOneToDevice((size_t)desc.width * desc.height * (requested ? requested : desc.channels),
                                            [&](uint8_t* dev, const int64_t* zero, int* st) {
                    return gamut_hip_qoi_decode_batch_device(&bytes, &size, 1, requested, zero, dev, &desc, st, nullptr);
                });
        } else decoded = (uint8_t*)gamut_hip_qoi_decode(bytes, (int)len, &desc, requested);
        if (!decoded) { error(kStrImageDecodingFailed); return; }
        if (!imageIsValidSize(1, (int)desc.width, (int)desc.height)) { error(kStrImageTooLarge); release(decoded); return; }
        const int comps = requested == 0 ? desc.channels : requested;
        // DEVIATION: the reference sets _pitch = desc.channels * desc.width (:133), the FILE's channel count, even when the
        // decoder was asked for another one; rows are then read at the wrong pitch (and past the buffer for RGBA files
        // loaded without alpha).  The pitch of the decoded buffer is used here.
        adopt(decoded, (int)desc.width, (int)desc.height, comps == 3 ? GAMUT_PIXEL_rgb8 : GAMUT_PIXEL_rgba8, comps, -1.0f, -1.0f);
        _layoutConstraints = 0;
        convertTo(applyLoadFlags(_type, flags), flags & 0xFFFF);
    }
    void loadQOIX(const uint8_t* bytes, size_t len, int flags)                              // plugins/qoix.d:64-146
    {
        const int requested = computeRequestedImageComponents(flags);                       // :92-99: only its verdict is used
        if (requested == 0) { error(kStrInvalidFlags); return; }
        gamut_hip_qoix_info hd, info;
        // qoix_lz4_decode :112: the flags are only validated, decodedType = streamType; a sub-codec that is not built (10-bit) or not
        // switched on (8-bit grey, gamut_hip_qoix_set_plane) fails the same way.  Switched on, l8 / la8 files take this path unchanged.
        if (!validLoadFlags(flags) || gamut_hip_qoix_read_header(bytes, len, &hd) != GAMUT_HIP_OK) { error(kStrImageDecodingFailed); return; }
        const int comps = hd.channels;
        uint8_t* decoded = decodeOne((size_t)hd.width * hd.height * comps, [&](uint8_t* dev, const int64_t* zero, int* st) {
            return gamut_hip_qoix_decode_batch_device(&bytes, &len, 1, 0, zero, dev, &info, st, nullptr);
        });
        if (!decoded) { error(kStrImageDecodingFailed); return; }
        if (!imageIsValidSize(1, hd.width, hd.height)) { error(kStrImageTooLarge); release(decoded); return; }     // :122-127
        adopt(decoded, hd.width, hd.height, hd.pixel_type, comps, hd.pixel_aspect_ratio, hd.resolution_y);          // :129-142, pitch = width * channels
        _layoutConstraints = 0;                                                             // :135
        convertTo(applyLoadFlags(_type, flags), flags & 0xFFFF);                           // :145
    }
    void loadBMP(const uint8_t* bytes, size_t len, int flags)                               // plugins/bmp.d:85-163
    {
        int requested = computeRequestedImageComponents(flags);
        if (requested == 0) { error(kStrInvalidFlags); return; }
        if (requested == -1) requested = 0;
        gamut_hip_bmp_info hd, info;
        if (gamut_hip_bmp_read_header(bytes, len, &hd) != GAMUT_HIP_OK) { error(kStrImageDecodingFailed); return; }
        const int comps = requested ? requested : hd.channels_in_file;
        uint8_t* decoded = decodeOne((size_t)hd.width * hd.height * comps, [&](uint8_t* dev, const int64_t* zero, int* st) {
            return gamut_hip_bmp_decode_batch_device(&bytes, &len, 1, requested, zero, dev, &info, st, nullptr);
        });
        if (!decoded) { error(kStrImageDecodingFailed); return; }
        if (!imageIsValidSize(1, info.width, info.height)) { error(kStrImageTooLarge); release(decoded); return; }
        adopt(decoded, info.width, info.height, kType8[comps], comps, info.pixel_aspect_ratio == -1 ? -1.0f : info.pixel_aspect_ratio,
              info.pixels_per_meter_y == -1 ? -1.0f : info.pixels_per_meter_y / kInchesPerMeter);          // :134-135
        convertTo(applyLoadFlags(_type, flags), flags & 0xFFFF);
    }
    void loadTGA(const uint8_t* bytes, size_t len, int flags)                               // plugins/tga.d:42-95
    {
        gamut_hip_tga_info hd, info;
        const int hrc = gamut_hip_tga_read_header(bytes, len, &hd);
        if (!hd.detected) { error(kStrImageDecodingFailed); return; }                       // getImageInfo :51-55
        if (!imageIsValidSize(1, hd.width, hd.height)) { error(kStrImageTooLarge); return; } // :57-61
        if (hrc != GAMUT_HIP_OK) { error(kStrImageDecodingFailed); return; }                // decodeImage's header part :63-71
        const int comps = hd.channels_in_file;                                              // the file's own type; the flags act in convertTo
        uint8_t* decoded = decodeOne((size_t)hd.width * hd.height * comps, [&](uint8_t* dev, const int64_t* zero, int* st) {
            return gamut_hip_tga_decode_batch_device(&bytes, &len, 1, 0, zero, dev, &info, st, nullptr);
        });
        if (!decoded) { error(kStrImageDecodingFailed); return; }
        adopt(decoded, hd.width, hd.height, kType8[comps], comps, -1.0f, -1.0f);                // :87-88 GAMUT_UNKNOWN_ASPECT_RATIO / _RESOLUTION
        convertTo(applyLoadFlags(_type, flags), flags & 0xFFFF);                           // :94
    }
    void loadSQZ(const uint8_t* bytes, size_t len, int flags)                               // plugins/sqz.d:43-133
    {
        gamut_hip_sqz_info hd, info;
        // the sizing call :80-85: SQZ_decode_header and SQZ_validate_input; anything but SQZ_BUFFER_TOO_SMALL is an I/O failure
        if (gamut_hip_sqz_read_header(bytes, len, &hd) != GAMUT_HIP_OK) { error(kStrImageDecodingIOFailure); return; }
        const size_t nbytes = (size_t)hd.width * hd.height * hd.planes;
        if (hd.width > MAX_W || hd.height > MAX_H || (long long)nbytes > MAX_BYTES) { error(kStrImageTooLarge); return; }      // :88-94 (16-bit sides never get here)
        uint8_t* decoded = decodeOne(nbytes, [&](uint8_t* dev, const int64_t* zero, int* st) {                                   // :112-118
            return gamut_hip_sqz_decode_batch_device(&bytes, &len, 1, zero, dev, &info, st, nullptr);
        });
        if (!decoded) { error(kStrImageDecodingIOFailure); return; }
        adopt(decoded, hd.width, hd.height, hd.pixel_type, hd.planes, -1.0f, -1.0f);            // :120-129 l8 / rgb8, GAMUT_UNKNOWN_ASPECT_RATIO / _RESOLUTION
        _layoutConstraints = 0;                                                             // :127
        convertTo(applyLoadFlags(_type, flags), flags & 0xFFFF);                           // :132
    }
    // Layers of tight top-down rgba8 rows (device memory) into the image's own storage, whatever pitch and layer offset its constraints gave it
    bool fillLayersFromDevice(const uint8_t* dev, size_t layerBytes, size_t rowBytes)
    {
        if (!layerBytes || !_layerCount) return true;
        if (_device)                                                                         // one launch of the same-type scanline copy (k_copy_rows)
            return gamut_hip_scanlines_convert_device(_type, dev, (int64_t)rowBytes, (int64_t)layerBytes, _type, _data, _pitch, _layerOffset,
                                                      _width, _height, _layerCount, nullptr) == GAMUT_HIP_OK &&
                   gamut_hip_stream_synchronize(nullptr) == GAMUT_HIP_OK;
        std::vector<uint8_t> host(layerBytes * (size_t)_layerCount);
        if (gamut_hip_memcpy_d2h(host.data(), dev, host.size(), nullptr) != GAMUT_HIP_OK || gamut_hip_stream_synchronize(nullptr) != GAMUT_HIP_OK) return false;
        for (int l = 0; l < _layerCount; ++l)
            for (int y = 0; y < _height; ++y)
                memcpy(_data + (ptrdiff_t)l * _layerOffset + (ptrdiff_t)y * _pitch, host.data() + (size_t)l * layerBytes + (size_t)y * rowBytes, rowBytes);
        return true;
    }
    void loadGIF(const uint8_t* bytes, size_t len, int flags)                               // plugins/gif.d:57-103
    {
        gamut_hip_gif_info hd, info;
        if (gamut_hip_gif_read_header(bytes, len, &hd) != GAMUT_HIP_OK) { error(kStrImageDecodingFailed); return; }     // decoder.open: host only
        // createLayeredNoInit(width, height, numLayers, rgba8, cast(LayoutConstraints) flags) :77-81
        if (!createLayered(hd.width, hd.height, hd.layers, GAMUT_PIXEL_rgba8, flags & 0xFFFF, false)) return;
        _resolutionY = -1.0f; _pixelAspectRatio = hd.pixel_aspect_ratio;                   // :70-71
        const size_t layerBytes = (size_t)hd.width * hd.height * 4, nbytes = layerBytes * (size_t)hd.layers;
        if (nbytes) {
            // the decode is the GPU's either way: straight into a device image whose layers are tight, else through a staging allocation
            const bool direct = _device && _pitch == hd.width * 4 && (hd.layers <= 1 || (size_t)_layerOffset == layerBytes);
            uint8_t* dev = direct ? _data : dmalloc(nbytes);
            const int64_t zero = 0, cap = (int64_t)nbytes; int st = 0;
            bool ok = dev && gamut_hip_gif_decode_batch_device(&bytes, &len, 1, &zero, &cap, dev, &info, &st, nullptr) == GAMUT_HIP_OK;
            if (ok && !direct) ok = fillLayersFromDevice(dev, layerBytes, (size_t)hd.width * 4);
            if (dev && !direct) (void)hipFree(dev);
            if (!ok) { cleanupBitmapIfOwned(); error(kStrImageDecodingFailed); return; }
        }
        convertTo(applyLoadFlags(_type, flags), flags & 0xFFFF);                           // :102, over all layers
    }
};

namespace {

// ---- saving (image.d:940-1011): saveToStream -> g_plugins[fif].saveProc.  A saver states what its format refuses and names the codec's
// two calls on one image, the host drop-in and the device batch entry; encode_image, save_to_memory and save_to_file do the rest. ----
using Saver = uint8_t* (*)(gamut_image* img, int flags, size_t* len);           // -> the malloc'd file, *len bytes, or NULL: refused or failed

// a pixel type's channel count when it is one of l8 / la8 / rgb8 / rgba8 (l16 / la16 / rgb16 / rgba16 for channels16), else 0
int channels8(int type)
{
    return type == GAMUT_PIXEL_l8 ? 1 : type == GAMUT_PIXEL_la8 ? 2 : type == GAMUT_PIXEL_rgb8 ? 3 : type == GAMUT_PIXEL_rgba8 ? 4 : 0;
}
int channels16(int type) { return type % 3 == 1 ? channels8(type - 1) : 0; }

// a batch of one for a codec's *_encode_batch_device: the image's pixels where they are, the file at out_offset 0 of the thread's encode scratch
struct OneImage { const uint8_t* src; int64_t pitch, layer_offset, out_offset; uint8_t* out; int64_t len; int status; hipStream_t stream; };

// the malloc'd file a host drop-in returned, its int length handed over
uint8_t* host_file(void* file, int n, size_t* len)
{
    if (file) *len = (size_t)n;
    return (uint8_t*)file;
}
// One image through its codec, wherever its pixels live.  host(&n) is the codec's drop-in on the host pixels (it stages them through pinned
// memory); device(b) is the codec's batch entry on the batch of one `b`: device pixels are encoded where they are, into `bound` bytes of
// the thread's encode scratch, and the stream comes back in malloc memory.
template <class Host, class Device> uint8_t* encode_image(const gamut_image* img, size_t bound, size_t* len, Host host, Device device)
{
    if (!img->_device) { int n = 0; void* file = host(&n); return host_file(file, n, len); }
    OneImage b{ img->_data, img->_pitch, img->_layerOffset, 0, nullptr, 0, 0, thread_stream() };
    b.out = encode_staging(bound, 0, b.stream, nullptr);
    if (!b.out) return nullptr;
    if (device(b) != GAMUT_HIP_OK || b.len <= 0) return nullptr;
    uint8_t* r = (uint8_t*)malloc((size_t)b.len);
    if (!r) return nullptr;
    if (hipMemcpyAsync(r, b.out, (size_t)b.len, hipMemcpyDeviceToHost, b.stream) != hipSuccess || hipStreamSynchronize(b.stream) != hipSuccess) {
        (void)hipGetLastError(); free(r); return nullptr;
    }
    *len = (size_t)b.len;
    return r;
}

// saveQOI (plugins/qoi.d:149-184): rgb8 / rgba8, QOI_SRGB; flags ignored
uint8_t* save_qoi(gamut_image* img, int, size_t* len)
{
    gamut_hip_qoi_desc desc{};
    desc.width = (uint32_t)img->_width; desc.height = (uint32_t)img->_height; desc.colorspace = 0;
    desc.channels = channels8(img->_type);
    if (desc.channels < 3 || gamut_hip_qoi_encode_bound(&desc) == 0) return nullptr;                    // the bound is 0 for what qoi_encode refuses
    return encode_image(img, (size_t)gamut_hip_qoi_encode_bound(&desc), len,
        [&](int* n) { return gamut_hip_qoi_encode(img->_data, &desc, img->_pitch, n); },
        [&](OneImage& b) { return gamut_hip_qoi_encode_batch_device(&b.src, &b.pitch, &desc, 1, &b.out_offset, b.out, &b.len, &b.status, b.stream); });
}

// saveJPEG (plugins/jpeg.d:112-148): l8 -> 1 component, rgb8 -> 3, everything else (rgba8 included: stb would drop the alpha) refused;
// quality 90 (4:2:0); flags ignored
uint8_t* save_jpeg(gamut_image* img, int, size_t* len)
{
    const int32_t comp = channels8(img->_type), quality = 90, w = img->_width, h = img->_height;
    if ((comp != 1 && comp != 3) || gamut_hip_jpeg_encode_bound(w, h, comp, quality) == 0) return nullptr;
    return encode_image(img, (size_t)gamut_hip_jpeg_encode_bound(w, h, comp, quality), len,
        [&](int* n) -> void* {                                 // the stbi_write_jpg_to_func drop-in, as saveJPEG calls it
            struct Sink { std::vector<uint8_t> b; } sink;
            auto put = [](void* ctx, const void* data, int size) {
                Sink* s = (Sink*)ctx;
                try { s->b.insert(s->b.end(), (const uint8_t*)data, (const uint8_t*)data + size); } catch (...) { s->b.clear(); }
            };
            if (!gamut_hip_jpeg_write_to_func(put, &sink, w, h, comp, img->_data, (int)img->_pitch, quality) || sink.b.empty()) return nullptr;
            void* r = malloc(sink.b.size());
            if (r) { memcpy(r, sink.b.data(), sink.b.size()); *n = (int)sink.b.size(); }
            return r;
        },
        [&](OneImage& b) { return gamut_hip_jpeg_encode_batch_device(&b.src, &b.pitch, &w, &h, &comp, &quality, 1, &b.out_offset, b.out, &b.len, &b.status, b.stream); });
}

// savePNG (plugins/png.d:172-221): the eight integer types, flags read (:201-206), pitch passed through as stb's signed stride
uint8_t* save_png(gamut_image* img, int flags, size_t* len)
{
    const int32_t is16 = channels16(img->_type) != 0, comp = is16 ? channels16(img->_type) : channels8(img->_type);
    const int32_t force_filter = (flags & GAMUT_ENCODE_PNG_FILTER_FAST) ? 0 : -1, w = img->_width, h = img->_height;
    int32_t level = flags & 15;
    if (level == GAMUT_ENCODE_PNG_COMPRESSION_DEFAULT) level = GAMUT_ENCODE_PNG_COMPRESSION_5;
    level--;
    if (!comp || level < 0 || level > 10 || gamut_hip_png_encode_bound(w, h, comp, is16) == 0) return nullptr;
    return encode_image(img, (size_t)gamut_hip_png_encode_bound(w, h, comp, is16), len,
        [&](int* n) { return gamut_hip_png_write_to_mem(img->_data, (int)img->_pitch, w, h, comp, n, is16, force_filter, level); },
        [&](OneImage& b) { return gamut_hip_png_encode_batch_device(&b.src, &b.pitch, &w, &h, &comp, &is16, &force_filter, &level, 1, &b.out_offset, b.out, &b.len, &b.status, b.stream); });
}

// saveBMP (plugins/bmp.d:166-194) + write_bmp's density fields (bmpenc.d:63-74): rgb8 / rgba8, one layer, 1..32767 each way; flags ignored
uint8_t* save_bmp(gamut_image* img, int, size_t* len)
{
    const int32_t comp = channels8(img->_type), w = img->_width, h = img->_height;
    if (comp < 3 || img->_layerCount != 1 || gamut_hip_bmp_encode_bound(w, h, comp) == 0) return nullptr;
    // pixelsPerMeterY = convertMetersToInches(dotsPerInchY), X through the aspect ratio (image.d:314-361)
    int32_t ppm_x = 0, ppm_y = 0;
    if (img->_resolutionY != -1) {
        ppm_y = (int)roundf(img->_resolutionY * kInchesPerMeter);
        if (img->_pixelAspectRatio != -1) ppm_x = (int)roundf(img->_resolutionY * img->_pixelAspectRatio * kInchesPerMeter);
    }
    return encode_image(img, (size_t)gamut_hip_bmp_encode_bound(w, h, comp), len,
        [&](int* n) { return gamut_hip_bmp_write_to_mem(img->_data, (int)img->_pitch, w, h, comp, ppm_x, ppm_y, n); },
        [&](OneImage& b) { return gamut_hip_bmp_encode_batch_device(&b.src, &b.pitch, &w, &h, &comp, &ppm_x, &ppm_y, 1, &b.out_offset, b.out, &b.len, &b.status, b.stream); });
}

// saveGIF (plugins/gif.d:105-147): rgba8 only, every layer a frame of 7 centiseconds, maxBitDepth 16, alpha threshold 10; flags ignored
uint8_t* save_gif(gamut_image* img, int, size_t* len)
{
    const int32_t w = img->_width, h = img->_height, frames = img->_layerCount;
    if (img->_type != GAMUT_PIXEL_rgba8 || frames < 1) return nullptr;
    if (gamut_hip_gif_encode_bound(w, h, frames) == 0) return nullptr;
    return encode_image(img, (size_t)gamut_hip_gif_encode_bound(w, h, frames), len,
        [&](int* n) { return gamut_hip_gif_write_to_mem(img->_data, (int)img->_pitch, (int64_t)img->_layerOffset, w, h, frames, 7, 16, 10, n); },
        [&](OneImage& b) { return gamut_hip_gif_encode_batch_device(&b.src, &b.pitch, &b.layer_offset, &w, &h, &frames, nullptr, nullptr, nullptr, 1, &b.out_offset, b.out, &b.len, &b.status, b.stream); });
}

// saveTGA (plugins/tga.d:128-150): l8 / la8 / rgb8 / rgba8, scanptr(y) of layer 0 from the bottom row up, enableRLE = true; flags ignored
uint8_t* save_tga(gamut_image* img, int, size_t* len)
{
    const int32_t comp = channels8(img->_type), w = img->_width, h = img->_height;
    if (!comp || img->_layerCount < 1 || gamut_hip_tga_encode_bound(w, h, comp) == 0) return nullptr;
    return encode_image(img, (size_t)gamut_hip_tga_encode_bound(w, h, comp), len,
        [&](int* n) { return gamut_hip_tga_write_to_mem(img->_data, (int)img->_pitch, w, h, comp, 1, n); },
        [&](OneImage& b) { return gamut_hip_tga_encode_batch_device(&b.src, &b.pitch, &w, &h, &comp, nullptr, 1, &b.out_offset, b.out, &b.len, &b.status, b.stream); });
}

// saveQOIX (plugins/qoix.d:156-242), the 8-bit types: rgb8 / rgba8 / rgbap8 (colorspace 2) and, while the QOI-Plane switch is on
// (gamut_hip_qoix_set_plane; off, the bound refuses them), l8 / la8 / lap8 (colorspace 2); layer 0, the image's pixel aspect ratio and
// vertical DPI in the header, LZ4 when it is smaller; 16-bit types wait for their codec; flags ignored
uint8_t* save_qoix(gamut_image* img, int, size_t* len)
{
    gamut_hip_qoix_desc d{};
    d.width = img->_width; d.height = img->_height;
    d.channels = img->_type == GAMUT_PIXEL_rgbap8 ? 4 : img->_type == GAMUT_PIXEL_lap8 ? 2 : channels8(img->_type);
    d.colorspace = img->_type == GAMUT_PIXEL_rgbap8 || img->_type == GAMUT_PIXEL_lap8 ? 2 : 0;
    d.mode = 0;
    d.pixel_aspect_ratio = img->_pixelAspectRatio; d.resolution_y = img->_resolutionY;
    if (!d.channels || img->_layerCount < 1 || gamut_hip_qoix_encode_bound(&d) < 0) return nullptr;
    return encode_image(img, (size_t)gamut_hip_qoix_encode_bound(&d), len,
        [&](int* n) { return gamut_hip_qoix_write_to_mem(img->_data, (int)img->_pitch, &d, n); },
        [&](OneImage& b) { return gamut_hip_qoix_encode_batch_device(&b.src, &b.pitch, &d, 1, &b.out_offset, b.out, &b.len, &b.status, b.stream); });
}

// saveDDS (plugins/dds.d:47-216): l8 / la8 / rgb8 / rgba8, scanline(y) of layer 0, BC7 blocks behind a DX10 header; flags ignored
uint8_t* save_dds(gamut_image* img, int, size_t* len)
{
    const int32_t comp = channels8(img->_type), w = img->_width, h = img->_height;
    if (!comp || img->_layerCount < 1 || gamut_hip_dds_encode_bound(w, h, comp) == 0) return nullptr;
    return encode_image(img, (size_t)gamut_hip_dds_encode_bound(w, h, comp), len,
        [&](int* n) { return gamut_hip_dds_write_to_mem(img->_data, (int)img->_pitch, w, h, comp, n); },
        [&](OneImage& b) { return gamut_hip_dds_encode_batch_device(&b.src, &b.pitch, &w, &h, &comp, 1, &b.out_offset, b.out, &b.len, &b.status, b.stream); });
}

// saveSQZ (plugins/sqz.d:141-201): rgb8 only, sides of at least 8, scanptr(0) of layer 0; Oklab, 7 levels (clamped to what the size
// admits), chroma one round later, snake scan; the byte budget comes from the flags and the file is the bytes used, not the budget.
// false: refused.
bool sqz_encode_desc(const gamut_image* img, int flags, gamut_hip_sqz_encode_desc* d)
{
    const int w = img->_width, h = img->_height;
    if (w < 8 || h < 8 || w > 65535 || h > 65535 || img->_type != GAMUT_PIXEL_rgb8 || img->_layerCount < 1) return false;
    *d = gamut_hip_sqz_encode_desc{};
    d->width = w; d->height = h; d->color_mode = 2; d->levels = 7; d->scan_order = 1; d->subsampling = 1;
    d->budget = gamut_hip_sqz_budget_from_flags(w, h, flags);
    return true;
}
uint8_t* save_sqz(gamut_image* img, int flags, size_t* len)
{
    gamut_hip_sqz_encode_desc d;
    if (!sqz_encode_desc(img, flags, &d)) return nullptr;
    if (!img->_device) { int n = 0; void* file = gamut_hip_sqz_write_to_mem(img->_data, (int)img->_pitch, &d, &n); return host_file(file, n, len); }
    uint8_t* file = (uint8_t*)malloc((size_t)d.budget);               // a host buffer for either writer (gamut_hip_sqz_set_writer): the device writer's file is downloaded into it
    if (!file) return nullptr;
    const uint8_t* src = img->_data; const int64_t pitch = img->_pitch, off = 0; int64_t n = 0; int status = 0;
    if (gamut_hip_sqz_encode_batch_device(&src, &pitch, &d, 1, &off, file, &n, &status, nullptr) != GAMUT_HIP_OK) { free(file); return nullptr; }
    if (void* shrunk = realloc(file, (size_t)n)) file = (uint8_t*)shrunk;
    *len = (size_t)n;
    return file;
}

// saveSQZ with the file left in HBM: device-resident rgb8 images only (a host image has no business there: save_sqz_to_memory)
uint8_t* save_sqz_to_device(gamut_image* img, int flags, size_t* len)
{
    gamut_hip_sqz_encode_desc d;
    if (!img->_device || !sqz_encode_desc(img, flags, &d)) return nullptr;
    if (img->_deviceFile) { (void)hipFree(img->_deviceFile); img->_deviceFile = nullptr; }
    uint8_t* file = nullptr;
    if (hipMalloc((void**)&file, (size_t)d.budget) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    const uint8_t* src = img->_data; const int64_t pitch = img->_pitch, off = 0; int64_t n = 0; int status = 0;
    if (gamut_hip_sqz_encode_batch_to_device(&src, &pitch, &d, 1, &off, file, &n, &status, nullptr) != GAMUT_HIP_OK) { (void)hipFree(file); return nullptr; }
    img->_deviceFile = file;
    *len = (size_t)n;
    return file;
}

// the generic entry dispatches these three (image.d:966-980); every other format has entries of its own
Saver generic_saver(int fif)
{
    return fif == GAMUT_FORMAT_QOI ? save_qoi : fif == GAMUT_FORMAT_JPEG ? save_jpeg : fif == GAMUT_FORMAT_GIF ? save_gif : nullptr;
}

// what every gamut_image_save_*_to_memory is: the file in malloc memory, or NULL and *len = 0
uint8_t* save_to_memory(Saver save, gamut_image* img, int flags, size_t* len)
{
    if (len) *len = 0;
    if (!img || !len || !img->isValid() || !img->_data || !save) return nullptr;
    return save(img, flags, len);
}
// what every gamut_image_save_*_to_file is; nothing is created when the image is refused
int save_to_file(Saver save, gamut_image* img, const char* path, int flags)
{
    if (!path) return 0;
    size_t n = 0;
    uint8_t* encoded = save_to_memory(save, img, flags, &n);
    if (!encoded) return 0;
    FILE* f = fopen(path, "wb");
    bool ok = f && fwrite(encoded, 1, n, f) == n;
    if (f && fclose(f) != 0) ok = false;
    free(encoded);
    return ok;
}

} // namespace

static int identify(const uint8_t* b, size_t len)
{
    static const uint8_t png[8] = { 0x89, 0x50, 0x4e, 0x47, 0x0d, 0x0a, 0x1a, 0x0a };
    if (b && len >= 2 && b[0] == 0xFF && b[1] == 0xD8) return GAMUT_FORMAT_JPEG;            // detectJPEG plugins/jpeg.d:106-110
    if (b && len >= 8 && !memcmp(b, png, 8)) return GAMUT_FORMAT_PNG;                       // detectPNG plugins/png.d:165-169
    if (b && len >= 4 && !memcmp(b, "qoif", 4)) return GAMUT_FORMAT_QOI;                    // detectQOI plugins/qoi.d:144-148
    if (b && len >= 4 && !memcmp(b, "qoix", 4)) return GAMUT_FORMAT_QOIX;                   // detectQOIX plugins/qoix.d:149-153 ('o' cannot be a TGA colour-map type)
    if (b && len >= 6 && (!memcmp(b, "GIF87a", 6) || !memcmp(b, "GIF89a", 6))) return GAMUT_FORMAT_GIF;   // detectGIF plugins/gif.d:42-53
    if (gamut_hip_identify_format(b, len) == GAMUT_HIP_FORMAT_BMP) return GAMUT_FORMAT_BMP;  // detectBMP plugins/bmp.d:45-82
    if (b && len >= 1 && b[0] == 0xA5) return GAMUT_FORMAT_SQZ;                             // detectSQZ plugins/sqz.d:135-139: one byte; by format number behind BMP, before TGA
    if (gamut_hip_identify_format(b, len) == GAMUT_HIP_FORMAT_TGA) return GAMUT_FORMAT_TGA;  // detectTGA plugins/tga.d:97-126, last (image.d:1056)
    return GAMUT_FORMAT_unknown;
}

extern "C" {

int  gamut_convert_pixel_type(int type, int op) { return convertPixelType(type, op); }
int  gamut_apply_load_flags(int type, int flags) { return applyLoadFlags(type, flags); }
int  gamut_compute_requested_image_components(int flags) { return computeRequestedImageComponents(flags); }
int  gamut_valid_load_flags(int flags) { return validLoadFlags(flags); }
int  gamut_layout_constraints_valid(int c) { return layoutConstraintsValid(c); }
int  gamut_layout_constraints_compatible(int newer, int older) { return layoutConstraintsCompatible(newer, older); }
int  gamut_identify_format_from_memory(const uint8_t* bytes, size_t len) { return identify(bytes, len); }
void gamut_free_image_data(void* p) { free(p); }

gamut_image* gamut_image_new(void) { return new (std::nothrow) gamut_image(); }
void gamut_image_delete(gamut_image* img) { if (img) { img->cleanupBitmapIfOwned(); if (img->_deviceFile) (void)hipFree(img->_deviceFile); delete img; } }

int gamut_image_create(gamut_image* img, int w, int h, int type, int layout) { return img->createLayered(w, h, 1, type, layout, true); }
int gamut_image_create_layered(gamut_image* img, int w, int h, int layers, int type, int layout) { return img->createLayered(w, h, layers, type, layout, true); }
int gamut_image_create_no_init(gamut_image* img, int w, int h, int type, int layout) { return img->createLayered(w, h, 1, type, layout, false); }
int gamut_image_create_layered_no_init(gamut_image* img, int w, int h, int layers, int type, int layout) { return img->createLayered(w, h, layers, type, layout, false); }
int gamut_image_create_with_no_data(gamut_image* img, int w, int h, int type, int layout)   // image.d:760-789
{
    if (!img->forgetPreviousUsage(1, w, h)) return 0;
    if (!layoutConstraintsValid(layout)) { img->error(kStrIllegalLayoutConstraints); return 0; }
    img->_data = nullptr; img->_allocArea = nullptr; img->_type = type; img->_width = w; img->_height = h; img->_pitch = 0;
    img->_layoutConstraints = (uint16_t)layout; img->_layerCount = 1; img->_layerOffset = 0;
    return 1;
}
int gamut_image_create_view(gamut_image* img, void* data, int w, int h, int type, int pitch)  // image.d:697-752
{
    if (!img->forgetPreviousUsage(1, w, h)) return 0;
    if (!valid_type(type)) { img->error(kStrUnsupportedTypeConversion); return 0; }
    const int minPitch = kPixelSize[type] * w, absPitch = pitch >= 0 ? pitch : -pitch;
    if (absPitch < minPitch) { img->error(kStrOverlappingScanlines); return 0; }
    img->_data = (uint8_t*)data; img->_allocArea = nullptr; img->_type = type; img->_width = w; img->_height = h; img->_pitch = pitch;
    img->_layoutConstraints = GAMUT_LAYOUT_DEFAULT; img->_layerCount = 1; img->_layerOffset = 0;
    return 1;
}

int gamut_image_load_from_memory(gamut_image* img, const uint8_t* bytes, size_t len, int flags)  // image.d:886-901, 1751-1772
{
    img->cleanupBitmapAndTypeIfAny();
    img->clearError();
    switch (identify(bytes, len)) {
    case GAMUT_FORMAT_JPEG: img->loadJPEG(bytes, len, flags); break;
    case GAMUT_FORMAT_PNG:  img->loadPNG(bytes, len, flags); break;
    case GAMUT_FORMAT_QOI:  img->loadQOI(bytes, len, flags); break;
    case GAMUT_FORMAT_QOIX: img->loadQOIX(bytes, len, flags); break;
    case GAMUT_FORMAT_BMP:  img->loadBMP(bytes, len, flags); break;
    case GAMUT_FORMAT_GIF:  img->loadGIF(bytes, len, flags); break;
    case GAMUT_FORMAT_TGA:  img->loadTGA(bytes, len, flags); break;
    case GAMUT_FORMAT_SQZ:  img->loadSQZ(bytes, len, flags); break;
    default: img->error(kStrImageFormatUnidentified); break;
    }
    return img->isValid();
}

int gamut_image_convert_to(gamut_image* img, int targetType, int layout) { return img->convertTo(targetType, layout); }
int gamut_image_set_layout(gamut_image* img, int layout) { return img->convertTo(img->_type, layout); }
int gamut_image_convert_op(gamut_image* img, int op, int layout) { return img->convertTo(convertPixelType(img->_type, op), layout); }
int gamut_image_convert_to_greyscale_alpha(gamut_image* img, int layout)
{ return img->convertTo(convertPixelType(convertPixelType(img->_type, GAMUT_TO_GREYSCALE), GAMUT_TO_ADD_ALPHA), layout); }
int gamut_image_convert_to_rgba(gamut_image* img, int layout)
{ return img->convertTo(convertPixelType(convertPixelType(img->_type, GAMUT_TO_RGB), GAMUT_TO_ADD_ALPHA), layout); }
// in-place flips of every layer on the GPU (flip.hip): a device image as it lies, a host image layer by layer through the drop-in
static int flip_pixels(gamut_image* img, int vertical)
{
    if (img->_device)
        return gamut_hip_flip_device(img->_type, img->_data, img->_pitch, img->_layerOffset, img->_width, img->_height, img->_layerCount, vertical, nullptr) == GAMUT_HIP_OK &&
               gamut_hip_stream_synchronize(nullptr) == GAMUT_HIP_OK;
    for (int layer = 0; layer < img->_layerCount; ++layer)
        if (gamut_hip_flip(img->_type, img->_data + (ptrdiff_t)layer * img->_layerOffset, img->_pitch, img->_width, img->_height, vertical) != GAMUT_HIP_OK) return 0;
    return 1;
}
int gamut_image_flip_vertical(gamut_image* img)                                            // image.d:1524-1532
{
    if (!img->isValid()) return 0;
    if (!img->hasData()) return 1;
    if (img->_layoutConstraints & (GAMUT_LAYOUT_VERT_FLIPPED | GAMUT_LAYOUT_VERT_STRAIGHT))   // a constraint pins the storage order: flipVerticalPhysical :1926-1954, the rows swap places
        return flip_pixels(img, 1);
    if (img->_height >= 2) img->_data += (ptrdiff_t)img->_pitch * (img->_height - 1);        // flipVerticalLogical :1907-1924 (flipScanlinePointers)
    img->_pitch = -img->_pitch;
    return 1;
}
int gamut_image_flip_horizontal(gamut_image* img)                                          // image.d:1475-1509
{
    if (!img->isValid()) return 0;
    if (!img->hasData()) return 1;
    return flip_pixels(img, 0);
}

// layer / layerRange (image.d:645-679): a view, NOT owned, of layers [start, end) -- a 0-layer view is legal
gamut_image* gamut_image_layer_range(gamut_image* img, int layerStart, int layerEnd)
{
    gamut_image* res = new (std::nothrow) gamut_image();
    if (!res) return nullptr;
    if (!img->isValid() || !img->hasData() || layerStart > layerEnd || layerStart < 0 || layerEnd > img->_layerCount) return res;     // (asserts there): stays errored
    res->clearError();
    res->_data = img->_data + (ptrdiff_t)img->_layerOffset * layerStart;
    res->_allocArea = nullptr;
    res->_type = img->_type; res->_width = img->_width; res->_height = img->_height; res->_pitch = img->_pitch;
    res->_layoutConstraints = GAMUT_LAYOUT_DEFAULT;
    res->_layerCount = layerEnd - layerStart; res->_layerOffset = img->_layerOffset;
    res->_device = img->_device;
    return res;
}
// createLayeredView (image.d:706-752)
int gamut_image_create_layered_view(gamut_image* img, void* data, int w, int h, int layers, int type, int pitch, int layerOffsetBytes)
{
    if (!img->forgetPreviousUsage(layers, w, h)) return 0;
    if (!valid_type(type)) { img->error(kStrUnsupportedTypeConversion); return 0; }
    const int minPitch = kPixelSize[type] * w, absPitch = pitch >= 0 ? pitch : -pitch;
    if (absPitch < minPitch) { img->error(kStrOverlappingScanlines); return 0; }
    if (layers > 1) {
        if (layerOffsetBytes < 0) { img->error(kStrInvalidNegLayerOffset); return 0; }
        if ((long long)layerOffsetBytes < (long long)absPitch * h) { img->error(kStrOverlappingLayers); return 0; }
    }
    img->_data = (uint8_t*)data; img->_allocArea = nullptr; img->_type = type; img->_width = w; img->_height = h; img->_pitch = pitch;
    img->_layoutConstraints = GAMUT_LAYOUT_DEFAULT; img->_layerCount = layers; img->_layerOffset = (layers == 0 || layers == 1) ? 0 : layerOffsetBytes;
    return 1;
}
// copyPixelsTo (image.d:811-841): same size, type and layer count (asserts there; 0 here), both with pixels, both in host memory
// or both in HBM.  Rows go through the GPU copy path (K9, scanlinesCopy): one layered launch for device images.
int gamut_image_copy_pixels_to(gamut_image* img, gamut_image* dst)
{
    if (!img->isValid() || !dst->isValid() || !img->hasData() || !dst->hasData()) return 0;
    if (dst->_layerCount != img->_layerCount || dst->_width != img->_width || dst->_height != img->_height || dst->_type != img->_type || dst->_device != img->_device) return 0;
    if (img->_width == 0 || img->_height == 0 || img->_layerCount == 0) return 1;
    if (img->_device)
        return gamut_hip_scanlines_convert_device(img->_type, img->_data, img->_pitch, img->_layerOffset, dst->_type, dst->_data, dst->_pitch, dst->_layerOffset,
                                                  img->_width, img->_height, img->_layerCount, nullptr) == GAMUT_HIP_OK && gamut_hip_stream_synchronize(nullptr) == GAMUT_HIP_OK;
    for (int layer = 0; layer < img->_layerCount; ++layer)
        if (gamut_hip_scanlines_copy(img->_type, img->_data + (ptrdiff_t)layer * img->_layerOffset, img->_pitch,
                                     dst->_data + (ptrdiff_t)layer * dst->_layerOffset, dst->_pitch, img->_width, img->_height) != GAMUT_HIP_OK) return 0;
    return 1;
}
// clone (image.d:795-806): createLayeredNoInit with the same constraints, then copyPixelsTo; an errored image on failure
gamut_image* gamut_image_clone(gamut_image* img)
{
    gamut_image* r = new (std::nothrow) gamut_image();
    if (!r) return nullptr;
    if (!img->isValid() || !valid_type(img->_type)) return r;
    r->_device = img->_device;
    if (!r->createLayered(img->_width, img->_height, img->_layerCount, img->_type, img->_layoutConstraints, false)) return r;
    if (img->hasData() && !gamut_image_copy_pixels_to(img, r)) { r->cleanupBitmapIfOwned(); r->error(kStrImageDecodingFailed); }
    return r;
}

// ---- device-resident storage (not in the reference) ----
int gamut_image_set_device_storage(gamut_image* img, int on)        // only while the image owns no pixels
{
    if (img->_data) return 0;
    if (on && gamut_hip_device_count() < 1) return 0;
    img->_device = on != 0;
    return 1;
}
int gamut_image_is_device(const gamut_image* img) { return img->_device; }
// one layer into tightly packed host rows (dst_pitch >= scanline bytes), top-down in logical order, wherever the pixels live
int gamut_image_copy_pixels_to_host(gamut_image* img, int layer, void* dst, int64_t dst_pitch)
{
    if (!img->isValid() || !img->_data || !dst || layer < 0 || layer >= (img->_layerCount ? img->_layerCount : 1)) return 0;
    const int row = img->_width * kPixelSize[img->_type];
    if (dst_pitch < row) return 0;
    const uint8_t* src = img->_data + (ptrdiff_t)layer * img->_layerOffset;
    if (img->_height == 0 || row == 0) return 1;
    if (!img->_device) {
        for (int y = 0; y < img->_height; ++y) memcpy((uint8_t*)dst + (size_t)y * dst_pitch, src + (ptrdiff_t)img->_pitch * y, (size_t)row);
        return 1;
    }
    if (img->_pitch >= 0)
        return hipMemcpy2D(dst, (size_t)dst_pitch, src, (size_t)(img->_pitch ? img->_pitch : row), (size_t)row, (size_t)img->_height, hipMemcpyDeviceToHost) == hipSuccess;
    // stored upside down: the lowest address is the last logical row; copy, then the rows land reversed
    const uint8_t* low = src + (ptrdiff_t)img->_pitch * (img->_height - 1);
    uint8_t* last = (uint8_t*)dst + (size_t)(img->_height - 1) * dst_pitch;
    for (int y = 0; y < img->_height; ++y)
        if (hipMemcpy(last - (size_t)y * dst_pitch, low + (size_t)(-img->_pitch) * y, (size_t)row, hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return 1;
}

// ---- saving: the generic entry (image.d:953-980) and one pair per format that it does not dispatch (savePNG plugins/png.d:172-221, ...) ----
uint8_t* gamut_image_save_to_memory(gamut_image* img, int fif, int flags, size_t* len) { return save_to_memory(generic_saver(fif), img, flags, len); }
int gamut_image_save_to_file(gamut_image* img, int fif, const char* path, int flags) { return save_to_file(generic_saver(fif), img, path, flags); }
uint8_t* gamut_image_save_png_to_memory(gamut_image* img, int flags, size_t* len) { return save_to_memory(save_png, img, flags, len); }
int gamut_image_save_png_to_file(gamut_image* img, const char* path, int flags) { return save_to_file(save_png, img, path, flags); }
uint8_t* gamut_image_save_bmp_to_memory(gamut_image* img, int flags, size_t* len) { return save_to_memory(save_bmp, img, flags, len); }
int gamut_image_save_bmp_to_file(gamut_image* img, const char* path, int flags) { return save_to_file(save_bmp, img, path, flags); }
uint8_t* gamut_image_save_tga_to_memory(gamut_image* img, int flags, size_t* len) { return save_to_memory(save_tga, img, flags, len); }
int gamut_image_save_tga_to_file(gamut_image* img, const char* path, int flags) { return save_to_file(save_tga, img, path, flags); }
uint8_t* gamut_image_save_qoix_to_memory(gamut_image* img, int flags, size_t* len) { return save_to_memory(save_qoix, img, flags, len); }
int gamut_image_save_qoix_to_file(gamut_image* img, const char* path, int flags) { return save_to_file(save_qoix, img, path, flags); }
uint8_t* gamut_image_save_dds_to_memory(gamut_image* img, int flags, size_t* len) { return save_to_memory(save_dds, img, flags, len); }
int gamut_image_save_dds_to_file(gamut_image* img, const char* path, int flags) { return save_to_file(save_dds, img, path, flags); }
uint8_t* gamut_image_save_sqz_to_memory(gamut_image* img, int flags, size_t* len) { return save_to_memory(save_sqz, img, flags, len); }
int gamut_image_save_sqz_to_file(gamut_image* img, const char* path, int flags) { return save_to_file(save_sqz, img, path, flags); }
uint8_t* gamut_image_save_sqz_to_device(gamut_image* img, int flags, size_t* len) { return save_to_memory(save_sqz_to_device, img, flags, len); }
void gamut_free_encoded_image(void* encoded) { free(encoded); }                          // image.d:32-36

int   gamut_image_type(const gamut_image* img) { return img->_type; }
int   gamut_image_width(const gamut_image* img) { return img->_width; }
int   gamut_image_height(const gamut_image* img) { return img->_height; }
int   gamut_image_layers(const gamut_image* img) { return img->_layerCount; }
int   gamut_image_pitch_in_bytes(const gamut_image* img) { return img->_pitch; }
int   gamut_image_layer_offset_in_bytes(const gamut_image* img) { return img->_layerOffset; }
int   gamut_image_scanline_in_bytes(const gamut_image* img) { return valid_type(img->_type) ? img->_width * kPixelSize[img->_type] : 0; }
int   gamut_image_layout_constraints(const gamut_image* img) { return img->_layoutConstraints; }
int   gamut_image_is_error(const gamut_image* img) { return img->_error != nullptr; }
int   gamut_image_is_valid(const gamut_image* img) { return img->_error == nullptr; }
const char* gamut_image_error_message(const gamut_image* img) { return img->_error; }
int   gamut_image_has_data(const gamut_image* img) { return img->_data != nullptr; }
int   gamut_image_is_owned(const gamut_image* img) { return img->_data != nullptr && img->_allocArea != nullptr; }
int   gamut_image_is_stored_upside_down(const gamut_image* img) { return img->_pitch < 0; }
float gamut_image_pixel_aspect_ratio(const gamut_image* img) { return img->_pixelAspectRatio; }
float gamut_image_dots_per_inch_y(const gamut_image* img) { return img->_resolutionY; }
uint8_t* gamut_image_scanptr(gamut_image* img, int y) { return img->_data + (ptrdiff_t)img->_pitch * y; }
uint8_t* gamut_image_layerptr(gamut_image* img, int layer, int y) { return img->_data + (ptrdiff_t)img->_pitch * y + (ptrdiff_t)layer * img->_layerOffset; }
uint8_t* gamut_image_disown_data(gamut_image* img) { uint8_t* r = img->_allocArea; img->_allocArea = nullptr; return r; }

} // extern "C"
