// sqz_read_fuzz_host.cpp -- stand-alone mutation driver for the arithmetic of the device reader (gamut_amd/csrc/sqz_read.hpp): a
// SERIAL stand-in for the reader's workgroup -- the same walk, the same window steps with the lanes taken one after another, the
// same functions for flags, runs, advances, targets and the end rule -- decodes mutated and truncated files, and every coefficient
// is compared with the host front end (gamut_hip_sqz_decode_coeffs, gamut_amd/csrc/sqz_host.hip).  Built with that file alone under
// ASan + UBSan and run on the CPU (tools/sqz_read_fuzz_host.sh); no GPU, no Python.  Every input sits in a heap block of exactly its
// length and the coefficient buffer has exactly planes * w * h elements, so a read or write past either is an ASan report.  The
// stand-in runs with windows of 4, 64 and 1024 lanes: small windows put window boundaries inside the small files' passes.
//
//     sqz_read_fuzz_host <iterations per seed> <seed.sqz> ...
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../gamut_amd/csrc/sqz_write.hpp"
#include "../gamut_amd/csrc/sqz_read.hpp"

namespace gamut {                                                   // what sqz_host.hip takes from runtime.hip
static thread_local char g_err[512];
char* last_error_buf() { return g_err; }
int set_error(int status, const char* fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
    return status;
}
}
using namespace gamut;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return (uint32_t)(rng_state >> 16); }

struct Band {
    SqzBandGeom g; std::vector<uint32_t> lip, lsp;                  // entries are x | y << 16
    int bp = 0, mx = 0;
};

// the reader's kernel with `lanes` lanes, one lane after another
static void stand_in(const uint8_t* file, uint64_t len, const gamut_hip_sqz_info& I, int lanes, int16_t* coeffs)
{
    gamut_hip_sqz_encode_desc D{};
    D.width = I.width; D.height = I.height; D.color_mode = I.color_mode; D.levels = I.levels; D.scan_order = I.scan_order; D.subsampling = I.subsampling;
    SqzBandGeom g[kSqzSlots];
    sqz_band_geometry(D, g);
    std::vector<Band> bands(kSqzSlots);
    for (int s = 0; s < kSqzSlots; ++s) {
        bands[s].g = g[s];
        if (!g[s].width) continue;
        std::vector<uint16_t> xy((size_t)g[s].width * g[s].height * 2);
        if (sqz_scan_order(I.scan_order, (int)g[s].width, (int)g[s].height, xy.data()) != GAMUT_HIP_OK) { fprintf(stderr, "scan order failed\n"); exit(1); }
        bands[s].lip.resize(xy.size() / 2);
        for (size_t k = 0; k < bands[s].lip.size(); ++k) bands[s].lip[k] = xy[2 * k] | (uint32_t)xy[2 * k + 1] << 16;
    }
    const int64_t N = (int64_t)(len * 8u), window = 32 * (int64_t)lanes;
    auto coef = [&](const Band& b, uint32_t e) -> int16_t& { return coeffs[b.g.offset + (int64_t)(e >> 16) * b.g.stride + (e & 0xFFFFu)]; };
    int64_t pos = 48;
    const uint32_t planes = (uint32_t)I.planes, levels = (uint32_t)I.levels;
    uint32_t state = 0, plane = 0, level = 0, o = 0;
    int round = 0; bool done = false, stop = false;
    std::vector<uint32_t> fl((size_t)lanes);
    std::vector<uint64_t> sum((size_t)lanes);
    while (!done && pos < N && !stop) {
        done = true;
        for (;;) {
            Band& b = bands[(plane * kSqzLevels + level) * kSqzOrients + o];
            if (round < b.g.round || (round > b.g.round && b.bp == 0)) done = done && round > b.g.round;
            else {
                if (b.g.round == round) b.mx = b.bp = sqzr_nibble(file, len, &pos);
                const uint32_t n = (uint32_t)b.lip.size(), lspn = (uint32_t)b.lsp.size();
                std::vector<uint32_t> nsp;
                bool go = true;
                if (n != 0u && b.bp > 0) {
                    const uint32_t mask = 1u << b.bp;
                    const int64_t s = pos;
                    int64_t carry_prev = s - 1;
                    uint64_t carry_sum = 0;
                    bool closed = false;
                    for (int64_t P = s; P < N && !closed; P += window) {
                        // steps 1-3: every lane's flags, the flag in front of its first record, the sum of its advances
                        int64_t last = carry_prev;
                        std::vector<int64_t> pv((size_t)lanes);
                        for (int t = 0; t < lanes; ++t) {
                            const int64_t p = P + 32 * (int64_t)t;
                            fl[(size_t)t] = sqzr_flags(p < N ? sqzr_bits32(file, len, p) : 0u, p, s, N);
                            pv[(size_t)t] = last;
                            int64_t q = last;
                            sum[(size_t)t] = 0;
                            for (uint32_t rem = fl[(size_t)t]; rem; ) {
                                const int bit = __builtin_clz(rem);
                                rem &= ~(0x80000000u >> bit);
                                sum[(size_t)t] += sqzr_advance(sqzr_run(file, len, p + bit, q));
                                q = p + bit;
                            }
                            last = q;
                        }
                        // steps 4-5: targets from the prefix sums; the first overshoot ends the pass
                        uint64_t cum = carry_sum;
                        for (int t = 0; t < lanes && !closed; ++t) {
                            const int64_t p = P + 32 * (int64_t)t;
                            int64_t q = pv[(size_t)t];
                            for (uint32_t rem = fl[(size_t)t]; rem; ) {
                                const int bit = __builtin_clz(rem);
                                rem &= ~(0x80000000u >> bit);
                                cum += sqzr_advance(sqzr_run(file, len, p + bit, q));
                                if (cum - 1u >= (uint64_t)n) { pos = p + bit + 1; closed = true; break; }
                                const uint32_t e = b.lip[(size_t)(cum - 1u)];
                                b.lip[(size_t)(cum - 1u)] = kSqzrTaken;
                                nsp.push_back(e);
                                coef(b, e) = (int16_t)(uint16_t)((uint32_t)(uint16_t)coef(b, e) | mask | sqzr_sign(file, len, q));
                                q = p + bit;
                            }
                        }
                        carry_sum = cum; carry_prev = last;
                    }
                    if (!closed) pos = N;
                    go = pos < N;
                    if (go && !nsp.empty()) {
                        size_t w = 0;
                        for (size_t k = 0; k < b.lip.size(); ++k) if (b.lip[k] != kSqzrTaken) b.lip[w++] = b.lip[k];
                        b.lip.resize(w);
                    }
                }
                if (go) {
                    const uint64_t m = sqzr_refine_bits(lspn, pos, N);
                    const uint32_t rmask = 1u << (b.bp & 15);
                    for (uint64_t gq = 0; gq < (m + 31u) / 32u; ++gq) {
                        uint32_t w = sqzr_bits32(file, len, pos + (int64_t)(32u * gq));
                        const uint64_t valid = m - 32u * gq;
                        if (valid < 32u) w &= ~(0xFFFFFFFFu >> valid);
                        while (w) {
                            const int bit = __builtin_clz(w);
                            w &= ~(0x80000000u >> bit);
                            int16_t& c = coef(b, b.lsp[(size_t)(32u * gq) + (size_t)bit]);
                            c = (int16_t)(uint16_t)((uint32_t)(uint16_t)c | rmask);
                        }
                    }
                    pos += (int64_t)m;
                    go = m == (uint64_t)lspn && pos < N;
                }
                if (go) { b.bp -= b.bp > 0; b.lsp.insert(b.lsp.end(), nsp.begin(), nsp.end()); }
                if (!go) { stop = true; break; }
                done = done && b.bp == 0;
            }
            if (!state) {
                if (++o >= (uint32_t)kSqzOrients) {
                    ++level;
                    o = level < levels;
                    if (o == 0u) { level = 0; state = plane = planes > 1u; if (!state) break; }
                }
            } else if (++plane >= planes) {
                plane = 1;
                if (++o >= (uint32_t)kSqzOrients) {
                    ++level;
                    o = level < levels;
                    if (o == 0u) { level = 0; state = plane = 0; break; }
                }
            }
        }
        ++round;
    }
    for (Band& b : bands) {
        const uint32_t rm = sqzr_round_mask(b.mx, b.bp);
        if (rm) for (uint32_t e : b.lsp) coef(b, e) = (int16_t)(uint16_t)((uint32_t)(uint16_t)coef(b, e) | rm);
    }
}

int main(int argc, char** argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s <iterations per seed> <seed.sqz> ...\n", argv[0]); return 2; }
    const long iters = atol(argv[1]);
    long files = 0, compared = 0, refused = 0, skipped_large = 0;
    for (int s = 2; s < argc; ++s) {
        FILE* fh = fopen(argv[s], "rb");
        if (!fh) { fprintf(stderr, "cannot read %s\n", argv[s]); return 2; }
        std::vector<uint8_t> seed;
        for (int c; (c = fgetc(fh)) != EOF; ) seed.push_back((uint8_t)c);
        fclose(fh);
        for (long it = 0; it < iters; ++it) {
            std::vector<uint8_t> f = seed;
            const uint32_t kind = it == 0 ? 99 : rnd() % 7;
            if (kind == 0) f.resize(rnd() % (f.size() + 1));                                     // truncation, 0 bytes included
            else if (kind == 1) for (uint32_t k = 0, n = 1 + rnd() % 8; k < n && !f.empty(); ++k) f[rnd() % f.size()] ^= (uint8_t)(1u << (rnd() % 8));
            else if (kind == 2) for (uint32_t k = 0, n = 1 + rnd() % 4; k < n && !f.empty(); ++k) f[rnd() % f.size()] = (uint8_t)rnd();
            else if (kind == 3 && f.size() > 6) { f[5] = (uint8_t)rnd(); f[1 + rnd() % 4] = (uint8_t)(rnd() % 3 ? 0 : rnd()); }      // header fields: mode, levels, scan, sides
            else if (kind == 4 && f.size() > 8) {                                                    // endless runs, endless records, alternating tails
                static const uint8_t fill[4] = { 0x00, 0xFF, 0x55, 0xAA };
                const size_t a = 6 + rnd() % (f.size() - 6);
                memset(&f[a], fill[rnd() % 4], f.size() - a);
            }
            else if (kind == 5) { f.resize(6 + rnd() % 64); for (size_t k = 6; k < f.size(); ++k) f[k] = (uint8_t)rnd(); }           // a short random stream
            else if (kind == 6 && f.size() > 8) {                                                    // truncation plus a tail of its own
                f.resize(7 + rnd() % (f.size() - 7));
                const size_t extra = rnd() % 600;
                const uint32_t how = rnd() % 3;
                for (size_t k = 0; k < extra; ++k) f.push_back(how == 0 ? (uint8_t)rnd() : how == 1 ? 0x00 : 0xFF);
            }
            uint8_t* exact = (uint8_t*)malloc(f.size() ? f.size() : 1);
            if (!f.empty()) memcpy(exact, f.data(), f.size());
            gamut_hip_sqz_info info, info2;
            const int rc = gamut_hip_sqz_read_header(f.empty() ? nullptr : exact, f.size(), &info);
            ++files;
            if (rc == GAMUT_HIP_OK) {
                const size_t n = (size_t)info.width * info.height * info.planes;
                if (n > (size_t)1 << 20) ++skipped_large;                                            // header says gigabytes: the header verdict alone
                else {
                    int16_t* want = (int16_t*)malloc(n * sizeof(int16_t));
                    if (gamut_hip_sqz_decode_coeffs(exact, f.size(), want, n, &info2) != GAMUT_HIP_OK) { fprintf(stderr, "accepted header, refused stream: %s\n", last_error_buf()); return 1; }
                    static const int lanes[3] = { 4, 64, 1024 };
                    for (int l = 0; l < 3; ++l) {
                        int16_t* got = (int16_t*)calloc(n, sizeof(int16_t));
                        stand_in(exact, f.size(), info, lanes[l], got);
                        if (memcmp(got, want, n * sizeof(int16_t))) {
                            size_t k = 0;
                            while (got[k] == want[k]) ++k;
                            fprintf(stderr, "%s, iteration %ld (kind %u, %zu bytes), %d lanes: coefficient %zu is %d, the host front end has %d\n", argv[s], it, kind, f.size(), lanes[l], k, got[k], want[k]);
                            return 1;
                        }
                        free(got);
                    }
                    free(want);
                    ++compared;
                }
            } else ++refused;
            free(exact);
        }
    }
    printf("sqz_read_fuzz_host: %ld files, %ld decoded three ways and equal to the host front end, %ld refused by the header, %ld too large to decode here; no sanitizer report\n",
           files, compared, refused, skipped_large);
    return 0;
}
