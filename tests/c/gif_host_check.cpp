// gif_host_check.cpp -- a stand-alone program (its own main, no GPU, no Python) that feeds a corpus of GIF files to the host side of
// the GIF decoder, gamut_amd/csrc/gif_host.hip: gamut_hip_gif_read_header (container + code walk) and gif_parse as the batch decoder
// calls it (chain walk + the second pass that records frames, palettes, row maps and payloads).  Each file sits in a malloc block of
// exactly its length, so a sanitizer build sees any read past a file.  The corpus is what tools/gif_corpus.py writes: per file a
// little-endian u32 length and the bytes.  Built and run on the CPU, host code only:
//     python tools/gif_corpus.py corpus.bin
//     hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Igamut_amd/csrc tests/c/gif_host_check.cpp \
//           gamut_amd/csrc/gif_host.hip -o gif_host_check -fsanitize=address,undefined && ./gif_host_check corpus.bin
// It also fails when the chain walk refuses a file that the code walk accepts.  No test runs it.
#include "gif_host.hpp"
#include <cstdio>
namespace gamut {
static thread_local char g_err[512];
char* last_error_buf() { return g_err; }
int set_error(int status, const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); return status; }
}
extern "C" int gamut_hip_gif_read_header(const uint8_t*, size_t, gamut_hip_gif_info*);
int main(int argc, char** argv)
{
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    long n = 0, ok = 0, ok2 = 0, frames = 0;
    for (;;) {
        uint32_t len; if (fread(&len, 4, 1, f) != 1) break;
        uint8_t* buf = (uint8_t*)malloc(len ? len : 1);                 // exact size: ASan sees any read past the file
        if (len && fread(buf, 1, len, f) != len) return 3;
        gamut_hip_gif_info a, b; gamut::GifParsed p;
        int r1 = gamut_hip_gif_read_header(buf, len, &a);
        int r2 = gamut::gif_parse(buf, len, false, &p, &b);
        ok += r1 == 0; ok2 += r2 == 0; frames += (long)p.frames.size();
        if (r1 == 0 && r2 != 0) { printf("chain walk refuses what the code walk accepts: file %ld\n", n); return 4; }
        free(buf); ++n;
    }
    printf("%ld files, code walk accepts %ld, chain walk accepts %ld, %ld frames\n", n, ok, ok2, frames);
    return 0;
}
