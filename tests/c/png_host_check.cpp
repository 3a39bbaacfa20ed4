// png_host_check.cpp -- a stand-alone program (its own main, no GPU, no Python) for the host side of the PNG decoder,
// gamut_amd/csrc/png_file.hip: (a) the slice plans of the batch call's device inflate, (b) the gather of a stream's bytes from a file's
// IDAT chunks, (c) the chunk walk in its two forms (IDAT bytes copied / only located) on a corpus of files, each in a malloc block of
// exactly its length so that a sanitizer build sees any read past a file.  The corpus is what tests/png_host_corpus.py writes: per
// file a little-endian u32 length, a byte (1: also run every truncation of the file) and the bytes.
// tests/test_png_host_cpu.py builds it without a sanitizer and runs it.  With one, by hand, on the CPU, host code only:
//     python tests/png_host_corpus.py corpus.bin
//     hipcc -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Igamut_amd/csrc tests/c/png_host_check.cpp \
//           gamut_amd/csrc/png_file.hip -o png_host_check -fsanitize=address,undefined -lz && ./png_host_check corpus.bin
#include "png_file.hpp"
#include <cstdio>
#include <numeric>
#include <string>
namespace gamut {
static thread_local char g_err[512];
char* last_error_buf() { return g_err; }
int set_error(int status, const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof g_err, fmt, ap); va_end(ap); return status; }
}
using namespace gamut;

static long g_checks = 0;
#define CHECK(cond, ...) do { ++g_checks; if (!(cond)) { printf("FAILED %s:%d: %s -- ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); exit(1); } } while (0)

// ---- (a) slice plans ---------------------------------------------------------------------------------------------------------
static SlicePlan check_plan(const char* what, const std::vector<uint32_t>& len, int64_t slot, const SliceOverrides& ov)
{
    const size_t n = len.size();
    std::vector<int64_t> slot_bytes(n, slot);
    std::vector<int> streams(n);
    std::iota(streams.begin(), streams.end(), 0);
    const SlicePlan p = plan_slices(len, slot_bytes, streams, ov);
    CHECK(p.rounds >= 1 && p.rounds <= 32, "%s: %d rounds", what, p.rounds);
    CHECK(p.who.size() == n && p.len.size() == n && p.blob_off.size() == n && p.units_in_round.size() == (size_t)p.rounds, "%s: sizes", what);
    std::vector<char> seen(n, 0);
    for (size_t k = 0; k < n; ++k) {                       // `who`: every stream once, longest first, equal ones in file order
        CHECK(p.who[k] >= 0 && (size_t)p.who[k] < n && !seen[(size_t)p.who[k]], "%s: who[%zu]", what, k);
        seen[(size_t)p.who[k]] = 1;
        CHECK(p.len[k] == len[(size_t)p.who[k]], "%s: len[%zu]", what, k);
        if (k) CHECK(p.len[k - 1] > p.len[k] || (p.len[k - 1] == p.len[k] && p.who[k - 1] < p.who[k]), "%s: order at %zu", what, k);
    }
    // the units: round-major; those of a round are a prefix of `who`; per stream they tile [0, len) without a gap or an overlap
    std::vector<uint64_t> covered(n, 0); std::vector<int> units_of(n, 0), in_round((size_t)p.rounds, 0);
    int last_r = 0;
    for (const auto& u : p.units) {
        const int r = u.first; const size_t k = (size_t)u.second;
        CHECK(r >= last_r && r < p.rounds && k < n, "%s: unit (%d, %zu)", what, r, k);
        last_r = r;
        CHECK((int)k == in_round[(size_t)r], "%s: round %d is not a prefix of who at stream %zu", what, r, k);
        ++in_round[(size_t)r]; ++units_of[k];
        const uint64_t lo = (uint64_t)r * p.slice, hi = p.avail(r, k);
        CHECK(lo == covered[k] && hi >= lo && hi - lo <= p.slice && (hi > lo || p.len[k] == 0), "%s: unit (%d, %zu) covers [%llu, %llu) behind %llu", what, r, k,
              (unsigned long long)lo, (unsigned long long)hi, (unsigned long long)covered[k]);
        covered[k] = hi;
    }
    for (size_t k = 0; k < n; ++k) {
        CHECK(covered[k] == p.len[k], "%s: stream %zu covered to %llu of %u", what, k, (unsigned long long)covered[k], p.len[k]);
        if (p.len[k] == 0) CHECK(units_of[k] == 1 && p.units_in_round[0] > (int)k, "%s: empty stream %zu has %d units", what, k, units_of[k]);
        for (int r = 0; r < p.rounds; ++r) CHECK(p.avail(r, k) >= (r ? p.avail(r - 1, k) : 0) && p.avail(r, k) <= p.len[k], "%s: avail(%d, %zu) decreases", what, r, k);
        CHECK(p.avail(p.rounds - 1, k) == p.len[k], "%s: avail of stream %zu ends at %u of %u", what, k, p.avail(p.rounds - 1, k), p.len[k]);
    }
    for (int r = 0; r < p.rounds; ++r) CHECK(in_round[(size_t)r] == p.units_in_round[(size_t)r], "%s: units_in_round[%d]", what, r);
    // the staging image: the shares in the order of `who`, disjoint, inside blob_bytes; pitched: a round's slices are rows `pitch` apart
    uint64_t end = 0;
    for (size_t k = 0; k < n; ++k) {
        const uint64_t off = p.blob_off[(size_t)p.who[k]];
        CHECK(off >= end && off + p.len[k] <= p.blob_bytes, "%s: share of stream %zu at %llu, the one before ends at %llu, image %llu", what, k,
              (unsigned long long)off, (unsigned long long)end, (unsigned long long)p.blob_bytes);
        end = off + p.len[k];
        if (p.pitched) CHECK(off == k * p.pitch && off + (uint64_t)p.rounds * p.slice <= p.blob_bytes && p.pitch >= p.len[k], "%s: pitched share %zu", what, k);
    }
    if (ov.pitched >= 0) CHECK(p.pitched == (ov.pitched != 0), "%s: the layout override", what);
    return p;
}

static long check_plans()
{
    long plans = 0;
    const int64_t slots[2] = { 4096, 32 << 20 };           // small images; large ones (the plan then takes 512 KiB slices for short streams)
    for (int64_t slot : slots) for (uint32_t ov_slice : { 0u, 64u << 10 }) for (int ov_pitched : { -1, 0, 1 }) {
        SliceOverrides ov; ov.slice = ov_slice; ov.pitched = ov_pitched;
        const uint32_t s = check_plan("one byte", { 1 }, slot, ov).slice;                  // the slice the plan chooses for short streams
        CHECK(s == (ov_slice ? ov_slice : slot >= (16 << 20) ? 1u << 19 : 1u << 20), "base slice %u", s);
        const std::vector<std::vector<uint32_t>> sets = { { 0 }, { 1 }, { s - 1, s, s + 1 }, { 32 * s }, { 32 * s, 32 * s + 1 }, { 1, 40u << 20 }, { 0, 5, 0, s + 1, 0 } };
        for (const auto& set : sets) { check_plan("set", set, slot, ov); ++plans; }
        for (size_t n : { (size_t)1, (size_t)2, (size_t)256, (size_t)257 }) { check_plan("equal streams", std::vector<uint32_t>(n, 3 * s / 2), slot, ov); ++plans; }
        // at most 32 launches: streams of 8 MiB and more start from 1 MiB slices (or the override), doubled until 32 of them hold the longest
        uint32_t want = ov_slice ? ov_slice : 1u << 20;
        while ((uint64_t)want * 32 < (uint64_t)32 * s + 1) want *= 2;
        const SlicePlan edge = check_plan("32 s + 1", { 32 * s, 32 * s + 1 }, slot, ov);
        CHECK(edge.slice == want && edge.rounds == (int)(((uint64_t)32 * s + want) / want), "32 s + 1 bytes: slice %u, %d rounds", edge.slice, edge.rounds);
        const SlicePlan full = check_plan("32 s", { 32 * s }, slot, ov);
        CHECK((uint64_t)full.slice * (uint64_t)full.rounds == (uint64_t)32 * s && (s == (1u << 19) ? full.rounds == 16 : full.rounds == 32), "32 s bytes: slice %u, %d rounds", full.slice, full.rounds);
    }
    // arithmetic only, nothing is allocated: very unequal streams keep the tight layout, equal ones take the pitched one
    std::vector<uint32_t> unequal(300, 1); unequal.push_back(200u << 20);
    const SlicePlan t = check_plan("300 x 1 byte + 200 MiB", unequal, 4096, SliceOverrides{});
    CHECK(!t.pitched && t.who[0] == 300 && t.blob_bytes == (200u << 20) + 300 * 16, "300 x 1 byte + 200 MiB: pitched %d, image %llu", (int)t.pitched, (unsigned long long)t.blob_bytes);
    const SlicePlan q = check_plan("257 x 1 MiB", std::vector<uint32_t>(257, 1u << 20), 4096, SliceOverrides{});
    CHECK(q.pitched && q.slice == (1u << 20) && q.rounds == 1 && q.blob_bytes == (257ull << 20), "257 x 1 MiB: pitched %d", (int)q.pitched);
    return plans + 2;
}

// ---- (b) the gather ------------------------------------------------------------------------------------------------------------
struct Segmented {                                         // a payload cut into segments, each in a malloc block of exactly its length
    IdatSegments segments;
    Segmented(const std::vector<uint8_t>& payload, bool growing)
    {
        size_t at = 0;
        for (uint32_t n = 1; at < payload.size(); n += growing) {
            const uint32_t m = (uint32_t)std::min<size_t>(n, payload.size() - at);
            uint8_t* p = (uint8_t*)malloc(m);
            memcpy(p, payload.data() + at, m);
            segments.emplace_back(p, m); at += m;
        }
    }
    ~Segmented() { for (auto& s : segments) free(const_cast<uint8_t*>(s.first)); }
};
static long check_gather()
{
    std::vector<uint8_t> payload(1000);
    for (size_t i = 0; i < payload.size(); ++i) payload[i] = (uint8_t)(i * 131 + (i >> 8) * 17 + 1);
    long ranges = 0;
    for (int growing = 0; growing < 2; ++growing) {
        const Segmented sg(payload, growing != 0);
        CHECK(sg.segments.size() == (growing ? 45u : 1000u), "%zu segments", sg.segments.size());
        for (uint32_t skip : { 0u, 2u }) for (uint64_t w : { 1u, 7u, 64u })
            for (uint64_t lo = 0; lo + w + skip <= payload.size(); ++lo) {
                uint8_t* dst = (uint8_t*)malloc((size_t)w);
                memset(dst, 0xEE, (size_t)w);
                copy_idat_range(sg.segments, skip, lo, lo + w, dst);
                CHECK(!memcmp(dst, payload.data() + lo + skip, (size_t)w), "segments of %s, skip %u: bytes [%llu, %llu)", growing ? "1, 2, 3 .." : "1", skip,
                      (unsigned long long)lo, (unsigned long long)(lo + w));
                free(dst); ++ranges;
            }
    }
    return ranges;
}

// ---- (c) files ---------------------------------------------------------------------------------------------------------------------
struct Tally { long files = 0, accepted = 0, zlib_ok = 0, zlib_bad = 0, empty_idat = 0; };
static void check_file(const uint8_t* data, size_t len, Tally& t)
{
    uint8_t* buf = (uint8_t*)malloc(len ? len : 1);        // exact size: a sanitizer sees any read past the file
    memcpy(buf, data, len);
    PngHeader copied, located; IdatSegments segments;
    located.idat_segments = &segments;
    g_err[0] = 0; const int r1 = parse(buf, len, copied, false);  const std::string m1 = g_err;
    g_err[0] = 0; const int r2 = parse(buf, len, located, false); const std::string m2 = g_err;
    CHECK(r1 == r2 && m1 == m2, "file %ld (%zu bytes): verdict %d '%s' with the IDAT bytes copied, %d '%s' with them located", t.files, len, r1, m1.c_str(), r2, m2.c_str());
    CHECK(copied.ioff == located.ioff, "file %ld: ioff %u / %u", t.files, copied.ioff, located.ioff);
    CHECK(copied.x == located.x && copied.y == located.y && copied.depth == located.depth && copied.color == located.color && copied.img_n == located.img_n &&
          copied.pal_img_n == located.pal_img_n && copied.has_trans == located.has_trans && !memcmp(copied.palette, located.palette, 1024), "file %ld: headers differ", t.files);
    uint64_t total = 0;
    for (const auto& s : segments) { CHECK(s.second > 0 && s.first >= buf && s.first + s.second <= buf + len, "file %ld: a segment outside the file", t.files); total += s.second; }
    CHECK(total == located.ioff, "file %ld: segments hold %llu bytes, ioff %u", t.files, (unsigned long long)total, located.ioff);
    std::vector<uint8_t> gathered((size_t)total);
    copy_idat_range(segments, 0, 0, total, gathered.data());
    CHECK(total == 0 || (copied.idata && !memcmp(gathered.data(), copied.idata, (size_t)total)), "file %ld: the gathered bytes are not idata", t.files);
    if (r1 == GAMUT_HIP_OK) CHECK((copied.idata != nullptr) == (located.seen_idat && total > 0), "file %ld: idata / seen_idat", t.files);
    ++t.files;
    if (r1 == GAMUT_HIP_OK) ++t.accepted;
    if (r1 == GAMUT_HIP_OK && located.seen_idat && !total) ++t.empty_idat;      // (only empty IDAT chunks: "no IDAT" to one form, a short zlib header to the other)
    if (r1 == GAMUT_HIP_OK && copied.idata && !copied.is_iphone) {               // the zlib header as the walk of the batch call checks it == as inflate_idat does
        uint8_t hd[2] = { 0, 0 };
        copy_idat_range(segments, 0, 0, std::min<uint64_t>(total, 2), hd);
        const bool walk_ok = total >= 2 && zlib_header_ok(hd[0], hd[1]);
        HostBuf out; uint32_t out_len = 0;
        g_err[0] = 0;
        const uint8_t* r = inflate_idat(copied.idata, copied.ioff, (size_t)copied.defilter_bytes(), &out_len, true, out);
        const bool inflate_ok = r || strcmp(g_err, "png: bad zlib header") != 0;
        out.release();
        CHECK(walk_ok == inflate_ok, "file %ld: zlib header %02x %02x ok to the walk: %d, to inflate_idat: %d", t.files - 1, hd[0], hd[1], (int)walk_ok, (int)inflate_ok);
        ++(walk_ok ? t.zlib_ok : t.zlib_bad);
    }
    free(buf);
}

int main(int argc, char** argv)
{
    if (argc < 2) { printf("usage: png_host_check corpus.bin\n"); return 2; }
    const long plans = check_plans(), ranges = check_gather();
    FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
    Tally t; long whole = 0;
    std::vector<uint8_t> file;
    for (;;) {
        uint32_t len; uint8_t truncate;
        if (fread(&len, 4, 1, f) != 1) break;
        if (fread(&truncate, 1, 1, f) != 1) return 3;
        file.resize(len);
        if (len && fread(file.data(), 1, len, f) != len) return 3;
        check_file(file.data(), len, t); ++whole;
        for (size_t k = 0; truncate && k < len; ++k) check_file(file.data(), k, t);
    }
    fclose(f);
    printf("%ld slice plans, %ld gathered ranges, %ld files (%ld whole, the rest truncations): %ld accepted, zlib header ok %ld / bad %ld, %ld with empty IDAT chunks only; %ld checks\n",
           plans, ranges, t.files, whole, t.accepted, t.zlib_ok, t.zlib_bad, t.empty_idat, g_checks);
    return 0;
}
