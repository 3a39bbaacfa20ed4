// sqz_fuzz_host.cpp -- stand-alone mutation driver for the SQZ host front end (gamut_amd/csrc/sqz_host.hip): feeds mutated and
// truncated files to gamut_hip_sqz_read_header / gamut_hip_sqz_decode_coeffs.  Built with the host file alone under ASan + UBSan and
// run on the CPU (tools/sqz_fuzz_host.sh); no GPU, no Python.  Every input sits in a heap block of exactly its length and the
// coefficient buffer has exactly planes * w * h elements, so a read or write past either is an ASan report.
//
//     sqz_fuzz_host <iterations per seed> <seed.sqz> ...
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
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

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s <iterations per seed> <seed.sqz> ...\n", argv[0]); return 2; }
    const long iters = atol(argv[1]);
    long files = 0, accepted = 0, refused = 0, skipped_large = 0;
    for (int s = 2; s < argc; ++s) {
        FILE* fh = fopen(argv[s], "rb");
        if (!fh) { fprintf(stderr, "cannot read %s\n", argv[s]); return 2; }
        std::vector<uint8_t> seed;
        for (int c; (c = fgetc(fh)) != EOF; ) seed.push_back((uint8_t)c);
        fclose(fh);
        for (long it = 0; it < iters; ++it) {
            std::vector<uint8_t> f = seed;
            const uint32_t kind = it == 0 ? 99 : rnd() % 6;
            if (kind == 0) f.resize(rnd() % (f.size() + 1));                                     // truncation, 0 bytes included
            else if (kind == 1) for (uint32_t k = 0, n = 1 + rnd() % 8; k < n && !f.empty(); ++k) f[rnd() % f.size()] ^= (uint8_t)(1u << (rnd() % 8));
            else if (kind == 2) for (uint32_t k = 0, n = 1 + rnd() % 4; k < n && !f.empty(); ++k) f[rnd() % f.size()] = (uint8_t)rnd();
            else if (kind == 3 && f.size() > 6) { f[5] = (uint8_t)rnd(); f[1 + rnd() % 4] = (uint8_t)(rnd() % 3 ? 0 : rnd()); }      // header fields: mode, levels, scan, sides
            else if (kind == 4 && f.size() > 8) { const size_t a = 6 + rnd() % (f.size() - 6); memset(&f[a], rnd() & 1 ? 0x00 : 0xFF, f.size() - a); }   // endless runs / endless ones
            else if (kind == 5) { f.resize(6 + rnd() % 64); for (size_t k = 6; k < f.size(); ++k) f[k] = (uint8_t)rnd(); }           // a short random stream
            uint8_t* exact = (uint8_t*)malloc(f.size() ? f.size() : 1);
            if (!f.empty()) memcpy(exact, f.data(), f.size());
            gamut_hip_sqz_info info, info2;
            const int rc = gamut_hip_sqz_read_header(f.empty() ? nullptr : exact, f.size(), &info);
            ++files;
            if (rc == GAMUT_HIP_OK) {
                const size_t n = (size_t)info.width * info.height * info.planes;
                if (n > (size_t)1 << 22) ++skipped_large;                                            // header says gigabytes: the header verdict alone
                else {
                    int16_t* co = (int16_t*)malloc(n * sizeof(int16_t));
                    const int rc2 = gamut_hip_sqz_decode_coeffs(exact, f.size(), co, n, &info2);
                    if (rc2 != GAMUT_HIP_OK || memcmp(&info, &info2, sizeof(info))) { fprintf(stderr, "accepted header, refused stream: %s\n", gamut::last_error_buf()); return 1; }
                    free(co);
                    ++accepted;
                }
            } else ++refused;
            free(exact);
        }
    }
    printf("sqz_fuzz_host: %ld files, %ld decoded, %ld refused by the header, %ld too large to decode here; no sanitizer report\n", files, accepted, refused, skipped_large);
    return 0;
}
