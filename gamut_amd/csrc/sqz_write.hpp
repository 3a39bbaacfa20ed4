// sqz_write.hpp -- what the three SQZ encode files share: the band geometry and the scan orders (sqz_host.hip), the device writer
// (sqz_write.hip) and the batch calls above both writers (sqz_encode.hip).
#pragma once
#include "common.hpp"
#include <map>
#include <tuple>

namespace gamut {

// One subband as SQZ_common_init_context (codecs/sqz.d:1805-1827) lays it out: `offset` int16 elements from the image's first
// coefficient, rows `stride` elements apart, first visited in round `round`.  width == 0: the slot holds no band.
struct SqzBandGeom { int64_t offset; uint32_t width, height, stride; int32_t round; };
constexpr int kSqzPlanes = 3, kSqzLevels = 8, kSqzOrients = 4, kSqzSlots = kSqzPlanes * kSqzLevels * kSqzOrients;
// `d` has passed sqz_encode_check; g[(plane * 8 + level) * 4 + orientation], level 0 the coarsest
void sqz_band_geometry(const gamut_hip_sqz_encode_desc& d, SqzBandGeom g[kSqzSlots]);
// the width * height (x, y) pairs of a band's LIP in scan order 0..3 (raster, snake, Morton, Hilbert)
int  sqz_scan_order(int order, int width, int height, uint16_t* xy);
int  sqz_encode_check(gamut_hip_sqz_encode_desc* d);
int  sqz_encode_coeffs(const int16_t* planes, const gamut_hip_sqz_encode_desc& d, uint8_t* dst, int64_t* len);
int  sqz_undefined_shift_error();                                   // deviation (1): sets the message, returns GAMUT_HIP_ERR_INVALID_ARG

// The (x, y) tables of the bands' scans in DEVICE memory, x | y << 16 per position: what the device writer gathers through and the
// device reader (sqz_read.hip) fills its lists from.  Kept per thread and device, one per distinct (order, band width, band height),
// 4 bytes per coefficient of the band; a call that finds more than 1 GiB of them drops them all before it builds what it needs
// (every call ends with a wait on its stream, so nothing reads them then).
struct SqzScanTables {
    std::map<std::tuple<int, uint32_t, uint32_t>, uint32_t*> tables;
    size_t table_bytes = 0;
    void drop_tables();
    const uint32_t* table(int order, uint32_t w, uint32_t h);       // NULL with the thread's message when it cannot be had
};
SqzScanTables& sqz_scan_tables();                                   // the calling thread's, on the current device
constexpr size_t kSqzTableCap = 1ull << 30;

// The lowest-numbered refused image of a batch call, with the message it was refused with
struct SqzRefusals {
    int first_bad = -1, first_rc = GAMUT_HIP_OK; char first_msg[200] = { 0 };
    int* status;
    void refuse(int i, int rc)
    {
        if (status) status[i] = rc;
        if (first_bad < 0 || i < first_bad) { first_bad = i; first_rc = rc; snprintf(first_msg, sizeof(first_msg), "%s", last_error_buf()); }
    }
    int verdict() const { return first_bad >= 0 ? set_error(first_rc, "image %d: %s", first_bad, first_msg) : (int)GAMUT_HIP_OK; }
};

// The device writer.  For k in [0, which.size()): image i = which[k], descs[i] checked and clamped with a budget above 6, its
// coefficient buffer in DEVICE memory at coeffs + coeff_offset[i].  File i goes to out + out_offset[i] -- device memory when
// out_on_device, else host memory (the files alone are downloaded) -- and out_len[i] is its length; rcs[k] is the image's verdict
// (deviation (1) is the one refusal left at this point; such an image writes nothing and gets out_len 0).  Returns when the files are
// in place; anything but GAMUT_HIP_OK is a failure of the call, not of an image.
int sqz_write_files(const int16_t* coeffs, const int64_t* coeff_offset, const gamut_hip_sqz_encode_desc* descs, const std::vector<int>& which,
                    const int64_t* out_offset, uint8_t* out, bool out_on_device, int64_t* out_len, std::vector<int>& rcs, hipStream_t stream);

} // namespace gamut
