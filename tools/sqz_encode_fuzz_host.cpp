// sqz_encode_fuzz_host.cpp -- stand-alone driver for the SQZ host writer (gamut_amd/csrc/sqz_host.hip): feeds random and constructed
// coefficient buffers, geometries and byte budgets to gamut_hip_sqz_encode_coeffs.  Built with the host file alone under ASan + UBSan
// and run on the CPU (tools/sqz_encode_fuzz_host.sh); no GPU, no Python.  The coefficient buffer has exactly planes * w * h elements
// and the destination exactly `budget` bytes, each a heap block of its own, so a read or write past either is an ASan report.  A file
// that stayed below its budget is decoded again and must give the coefficients back.
//
//     sqz_encode_fuzz_host <iterations>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "../include/gamut_hip.h"

namespace gamut {                                                   // what sqz_host.hip takes from runtime.hip
static thread_local char g_err[512];
char* last_error_buf() { return g_err; }
int set_error(int status, const char* fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
    return status;
}
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }
static int16_t sm(int v) { return (int16_t)(v < 0 ? (-2 * v) | 1 : 2 * v); }

int main(int argc, char** argv)
{
    if (argc < 2) { fprintf(stderr, "usage: %s <iterations>\n", argv[0]); return 2; }
    const long iters = atol(argv[1]);
    long written = 0, lossless = 0, refused_args = 0, refused_shift = 0;
    for (long it = 0; it < iters; ++it) {
        gamut_hip_sqz_encode_desc d;
        d.width = 8 + (int)(rnd() % (it % 50 == 0 ? 600 : 72)); d.height = 8 + (int)(rnd() % (it % 50 == 0 ? 300 : 72));
        d.color_mode = (int)(rnd() % 4); d.levels = 1 + (int)(rnd() % 8); d.scan_order = (int)(rnd() % 4); d.subsampling = (int)(rnd() % 2);
        if (rnd() % 40 == 0) { const int w = (int)(rnd() % 5); if (w == 0) d.width = 7; else if (w == 1) d.height = 65536; else if (w == 2) d.color_mode = 4; else if (w == 3) d.scan_order = -1; else d.levels = 0; }
        const size_t n = (size_t)d.width * (size_t)d.height * (d.color_mode == 0 ? 1u : 3u);
        const bool valid = d.width >= 8 && d.width <= 65535 && d.height >= 8 && d.height <= 65535 && d.color_mode >= 0 && d.color_mode < 4 && d.scan_order >= 0 && d.levels >= 1;
        int16_t* co = (int16_t*)malloc((valid ? n : 8) * sizeof(int16_t));
        const uint32_t kind = rnd() % 7;
        bool small = true;                                                                       // no value is a negative short
        for (size_t k = 0; valid && k < n; ++k) {
            int v = 0;
            if (kind == 0) v = (int)(rnd() % 33) - 16;
            else if (kind == 1) v = (int)(rnd() % 4001) - 2000;
            else if (kind == 2) v = rnd() % 97 == 0 ? (int)(rnd() % 32767) - 16383 : 0;          // sparse: long runs
            else if (kind == 3) v = 0;
            else if (kind == 4) v = (int)(rnd() % 65536) - 32768;                                // the whole range of a short, the negative shorts among them
            else if (kind == 5) v = -16384 - (int)(rnd() % 16384);                               // nothing but negative shorts: the refused case
            else v = k == n / 2 ? 16383 : (int)(rnd() % 3) - 1;
            co[k] = sm(v);
            small = small && co[k] >= 0;
        }
        const uint32_t bk = rnd() % 4;
        d.budget = bk == 0 ? (int64_t)(rnd() % 12) : bk == 1 ? (int64_t)(7 + rnd() % 200) : bk == 2 ? (int64_t)(7 + rnd() % (n * 3 + 64)) : (int64_t)(n * 3 + 64);
        uint8_t* dst = (uint8_t*)malloc(d.budget > 0 ? (size_t)d.budget : 1);
        memset(dst, 0xC3, d.budget > 0 ? (size_t)d.budget : 1);
        int64_t len = -1;
        const int rc = gamut_hip_sqz_encode_coeffs(co, &d, dst, &len);
        if (rc == GAMUT_HIP_OK) {
            ++written;
            if (!valid || len < 7 || len > d.budget) { fprintf(stderr, "iteration %ld: length %lld of budget %lld\n", it, (long long)len, (long long)d.budget); return 1; }
            gamut_hip_sqz_info info;
            int16_t* back = (int16_t*)malloc(n * sizeof(int16_t));
            if (gamut_hip_sqz_decode_coeffs(dst, (size_t)len, back, n, &info) != GAMUT_HIP_OK || info.width != d.width || info.height != d.height || info.color_mode != d.color_mode) {
                fprintf(stderr, "iteration %ld: the written file is refused: %s\n", it, gamut::last_error_buf()); return 1;
            }
            if (len < d.budget && small) {
                ++lossless;
                if (memcmp(back, co, n * sizeof(int16_t))) { fprintf(stderr, "iteration %ld: %d x %d mode %d: the round trip differs\n", it, d.width, d.height, d.color_mode); return 1; }
            }
            free(back);
        } else {
            if (len != 0) { fprintf(stderr, "iteration %ld: refused with a length\n", it); return 1; }
            if (strstr(gamut::last_error_buf(), "1u << 32")) ++refused_shift; else ++refused_args;
            if (valid && d.budget > 6 && small) { fprintf(stderr, "iteration %ld: refused without a reason: %s\n", it, gamut::last_error_buf()); return 1; }
        }
        free(dst);
        free(co);
    }
    printf("sqz_encode_fuzz_host: %ld buffers, %ld files written (%ld below their budget and decoded back to their coefficients), %ld refused for their arguments, "
           "%ld for a band of nothing but negative shorts; no sanitizer report\n", iters, written, lossless, refused_args, refused_shift);
    return 0;
}
