// sqz_host.hip -- the SQZ front end on the host: SQZ_decode (source/gamut/codecs/sqz.d:2253-2296) restated up to and including
// SQZ_decode_round_coefficients (:2082-2103), and the back half of SQZ_encode (:2208-2240): SQZ_encode_header and SQZ_schedule_task over
// the coefficient buffer the GPU's front half (sqz_encode.hip) leaves.  Host code only: no device is needed or touched.
//
// SQZ is an embedded bit-plane coder (WDR: wavelet difference reduction): ONE bit stream, three linked lists per subband (LIP
// insignificant, NSP newly significant, LSP significant) and a scheduler that interleaves the subbands round by round.  The chain
// of (band, bit plane) segments is serial -- where one ends is known only once it has been read -- so this file walks a file bit by
// bit and the batch call (sqz.hip) runs one file per host thread; INSIDE a segment every bit position can be classified without its
// neighbours, which is what the device reader (sqz_read.hip, sqz_read.hpp) is built on.  What leaves this file is the reference's
// coefficient buffer as it stands before SQZ_dwt_convert_from_sign_magnitude: int16 sign-magnitude values (bit 0 the sign), planes
// one after another, subbands interleaved in place (SQZ_common_init_context :1798-1829).
//
// Kept from the reference, to the letter:
//   - header: 48 bits, and the verdict is !eob AFTER the last bit (:1913-1926), so a file of exactly 6 bytes is refused;
//   - SQZ_validate_input in read-only mode (:2170-2197): sides 8..65535, levels <= min(ilog2(min side) - 3, 8) with ilog2 = bsr + 1
//     (a side of 8..15 admits ONE level, 16..31 two, ...);
//   - the 4-bit max_bitplane read may give -1 at the end of the buffer (:1896); the sorting pass is skipped when bitplane <= 0 or the LIP
//     is empty (:1991); the WDR run is `run += run + bit` in 32 unsigned bits (:1948) and may wrap; a run past the LIP ends the pass;
//   - list order: exchange appends at the tail (:739-768), NSP is merged behind LSP only after a COMPLETED bit plane (:2070-2080): a pass
//     cut short by the end of the stream leaves its NSP unmerged and those coefficients are not rounded;
//   - coefficients are 16 bits: 1 << 15 is the sign bit of a short (:1998, :2044);
//   - every read is guarded by eob (:625-676): there is no read past the buffer, so no deviation is needed for that.
// REFUSALS the reference does not have: an allocation that cannot be had is GAMUT_HIP_ERR_OUT_OF_MEMORY (the reference tests its
// callocs the same way and returns SQZ_OUT_OF_MEMORY); a `capacity` below planes * w * h is GAMUT_HIP_ERR_INVALID_ARG.  A header
// field read as -1 at the end of the buffer is never used as an index (the reference would index SQZ_number_of_planes with it before
// it looks at eob; the verdict is the same).
#include "common.hpp"
#include "sqz_write.hpp"
#include <cmath>

namespace gamut {
namespace {

constexpr int kMaxLevel = 8, kBands = 4;

struct BitReader {                                                  // SQZ_bit_buffer_t :163-169, read side :625-676
    const uint8_t *ptr, *eob; uint32_t index = 0;
    bool at_end() const { return ptr >= eob; }
    int bit()
    {
        if (at_end()) return -1;
        const int b = (*ptr >> (7u - index)) & 1;
        if (index < 7u) ++index; else { ++ptr; index = 0; }
        return b;
    }
    int bits(uint32_t width)
    {
        uint32_t v = 0;
        for (;;) {
            if (at_end()) return -1;
            const uint32_t avail = 8u - index;
            if (avail >= width) {
                v = (v << width) | ((*ptr >> (avail - width)) & ((1u << width) - 1u));
                index += width;
                if (index > 7u) { ++ptr; index = 0; }
                return (int)v;
            }
            v = (v << avail) | (*ptr & ((1u << avail) - 1u));
            ++ptr; index = 0; width -= avail;
        }
    }
};

struct Node { uint16_t x, y; int32_t next; };                       // SQZ_list_node_t :172-177
struct List { int32_t head = -1, tail = -1; size_t length = 0; };
struct Band {                                                       // SQZ_dwt_subband_t :327-340
    Node* nodes = nullptr; size_t capacity = 0, used = 0;
    List lip, lsp, nsp;
    int16_t* data = nullptr; size_t width = 0, height = 0, stride = 0;
    int max_bitplane = 0, bitplane = 0, round = 0;
    ~Band() { free(nodes); }
    void add(List& l, size_t x, size_t y)                           // SQZ_list_add :704-727
    {
        if (used >= capacity) return;
        const int32_t k = (int32_t)used++;
        if (l.head < 0) l.head = k; else if (l.tail >= 0) nodes[l.tail].next = k;
        l.tail = k; ++l.length;
        nodes[k] = Node{ (uint16_t)x, (uint16_t)y, -1 };
    }
    int32_t exchange(List& src, List& dst, int32_t node, int32_t prev)      // :739-768
    {
        const int32_t next = nodes[node].next;
        if (prev >= 0) nodes[prev].next = next; else src.head = next;
        --src.length;
        if (dst.head < 0) dst.head = node; else if (dst.tail >= 0) nodes[dst.tail].next = node;
        dst.tail = node; ++dst.length;
        nodes[node].next = -1;
        return next;
    }
    void merge(List& src, List& dst)                                // :777-794
    {
        if (src.head < 0) return;
        if (dst.tail >= 0) nodes[dst.tail].next = src.head; else dst.head = src.head;
        dst.tail = src.tail; dst.length += src.length;
        src = List{};
    }
    int16_t& at(int32_t node) { return data[nodes[node].y * stride + nodes[node].x]; }
};

uint32_t ilog2(uint32_t x) { return x ? 32u - (uint32_t)__builtin_clz(x) : 0u; }         // :493-502: bsr + 1
uint32_t deinterleave(uint32_t i)                                   // :533-541
{
    i &= 0x55555555u; i = (i ^ (i >> 1)) & 0x33333333u; i = (i ^ (i >> 2)) & 0x0F0F0F0Fu;
    i = (i ^ (i >> 4)) & 0x00FF00FFu; i = (i ^ (i >> 8)) & 0x0000FFFFu;
    return i;
}
int iabs(int x) { return x < 0 ? -x : x; }
int isign(int x) { return x < 0 ? -1 : x > 0 ? 1 : 0; }

// ---- the four scan orders: each next() is the reference's scan function, the position in x, y ----
struct Scan { size_t x = 0, y = 0; };
struct Snake : Scan {                                               // SQZ_snake_scan_context_t :216-273, init :873-940, step :823-871
    size_t tile_x = 0, tile_y = 0, tile_w, tile_h, cols_rem, rows_rem, def_w, def_h;
    int r2l = 0;
    size_t grid_x = 0, grid_y = 0, grid_w, grid_h, col_index = 0;
    int col_odd = 0, row_odd = 0;
    size_t off_x = 0, off_y = 0;
    Snake(size_t width, size_t height, size_t tw, size_t th)
    {
        if (tw > width) tw = width;
        if (th > height) th = height;
        int step = 1;
        for (;;) {                                                  // an odd number of grid columns
            grid_w = (width + tw - 1u) / tw;
            if (grid_w & 1u) break;
            tw += (size_t)(ptrdiff_t)step;
            if (tw > width) tw = width; else if (tw == 0u) tw = 1u;
            step = -(iabs(step) + 1) * ((step > 0) - (step < 0));
        }
        cols_rem = width % tw;
        if (cols_rem == 0u) cols_rem = tw;
        tile_w = (grid_w > 1u || cols_rem > 0u) ? tw : cols_rem;
        def_w = tw;
        step = 2;
        for (;;) {                                                  // the last grid row's tiles have an odd number of rows
            rows_rem = height % th;
            if (rows_rem > 0u && !(rows_rem & 1u)) {
                th += (size_t)(ptrdiff_t)step;
                if (th > height) th = height; else if (th == 0u) th = 1u;
                step = -(iabs(step) + 2) * ((step > 0) - (step < 0));
            } else { if (rows_rem == 0u) rows_rem = th; break; }
        }
        grid_h = (height + th - 1u) / th;
        tile_h = (grid_h > 1u || rows_rem > 0u) ? th : rows_rem;
        def_h = th;
    }
    bool next()
    {
        enum { kColumns, kRows, kGridColumns } go;
        if (++tile_x < tile_w) go = kColumns;
        else {
            tile_x = 0;
            if (++tile_y < tile_h) go = kRows;
            else {
                tile_y = 0;
                if (++col_index < grid_w) go = kGridColumns;
                else {
                    col_index = 0;
                    if (++grid_y >= grid_h) return false;
                    row_odd = (int)(grid_y & 1u);
                    tile_h = grid_y < grid_h - 1u ? def_h : rows_rem;
                    off_y = grid_y * def_h;
                    go = kGridColumns;
                }
            }
        }
        if (go == kGridColumns) {
            const size_t last = grid_w - 1u;
            grid_x = row_odd ? last - col_index : col_index;
            col_odd = (int)(grid_x & 1u);
            tile_w = grid_x < last ? def_w : cols_rem;
            off_x = grid_x * def_w;
            go = kRows;
        }
        if (go == kRows) {
            const size_t row = col_odd ? (tile_h - 1u) - tile_y : tile_y;
            r2l = (int)((grid_y ^ row) & 1u);
        }
        x = (r2l ? (tile_w - 1u) - tile_x : tile_x) + off_x;
        y = (col_odd ? (tile_h - 1u) - tile_y : tile_y) + off_y;
        return true;
    }
};
struct Morton : Scan {                                              // :278-284, init :968-989, step :942-966
    size_t range, mask, index = 0, length, width, height;
    Morton(size_t w, size_t h) : width(w), height(h)
    {
        range = ilog2((uint32_t)(w > h ? h : w) - 1u);
        mask = (size_t)((1ull << (range * 2u)) - 1u);
        length = (size_t)(1ull << (range + ilog2((uint32_t)(w > h ? w : h) - 1u)));
    }
    bool next()
    {
        do {
            ++index;
            x = deinterleave((uint32_t)(index & mask));
            y = deinterleave((uint32_t)((index >> 1u) & mask));
            const uint32_t m = (uint32_t)((index & ~mask) >> range);
            if (width > height) x |= m; else y |= m;
            if (x < width && y < height) return true;
        } while (index < length);
        return false;
    }
};
struct Hilbert : Scan {                                             // :287-317, init :1094-1119, step :1013-1092 (the generalised curve for rectangles)
    struct Item { int x, y, ax, ay, bx, by; } items[32];
    int top = 0, width = 0, height = 0, dax = 0, day = 0, dbx = 0, dby = 0, index = -1;
    void push(int x_, int y_, int ax, int ay, int bx, int by) { items[top++] = Item{ x_, y_, ax, ay, bx, by }; }
    Hilbert(size_t w, size_t h)
    {
        if (w >= h) push(0, 0, (int)w, 0, 0, (int)h); else push(0, 0, 0, (int)h, (int)w, 0);
        next();                                                     // the first position, as SQZ_scan_init_hilbert_context does
    }
    bool next()
    {
        for (;;) {
            if (top == 0) return false;
            Item& it = items[top - 1];
            if (index < 0) {
                width = iabs(it.ax + it.ay); height = iabs(it.bx + it.by);
                dax = isign(it.ax); day = isign(it.ay); dbx = isign(it.bx); dby = isign(it.by);
                index = 0;
            }
            if (height == 1 || width == 1) {
                const bool along_a = height == 1;
                if (index < (along_a ? width : height)) {
                    x = (size_t)it.x; y = (size_t)it.y;
                    it.x += along_a ? dax : dbx; it.y += along_a ? day : dby;
                    ++index;
                    return true;
                }
                --top; index = -1;
                continue;
            }
            const Item cur = it;
            --top; index = -1;
            int ax2 = cur.ax / 2, ay2 = cur.ay / 2, bx2 = cur.bx / 2, by2 = cur.by / 2;
            const int w2 = iabs(ax2 + ay2), h2 = iabs(bx2 + by2);
            if (2 * width > 3 * height) {
                if ((w2 % 2) != 0 && width > 2) { ax2 += dax; ay2 += day; }
                push(cur.x + ax2, cur.y + ay2, cur.ax - ax2, cur.ay - ay2, cur.bx, cur.by);
                push(cur.x, cur.y, ax2, ay2, cur.bx, cur.by);
            } else {
                if ((h2 % 2) != 0 && height > 2) { bx2 += dbx; by2 += dby; }
                push(cur.x + (cur.ax - dax) + (bx2 - dbx), cur.y + (cur.ay - day) + (by2 - dby), -bx2, -by2, -(cur.ax - ax2), -(cur.ay - ay2));
                push(cur.x + bx2, cur.y + by2, cur.ax, cur.ay, cur.bx - bx2, cur.by - by2);
                push(cur.x, cur.y, bx2, by2, ax2, ay2);
            }
        }
    }
};

template <class S> void fill_lip(Band& b, S& s) { do b.add(b.lip, s.x, s.y); while (s.next()); }      // SQZ_common_init_subband :1860-1862

// SQZ_schedule :374-490 as a formula: plane 0 starts level l's bands at 0, l + 1, l + 1, l + 2; the chroma planes one round later, except
// that their levels above 0 have no LL band (entry 0, never visited)
int schedule(int mode, int plane, int level, int o)
{
    static const int first[4] = { 0, 1, 1, 2 };
    if (plane == 0) return o == 0 ? 0 : first[o] + level;
    if (mode == 0) return 0;
    if (level == 0) return first[o] + 1;
    return o == 0 ? 0 : first[o] + level + 1;
}

// What SQZ_encode and SQZ_decode share: the context, the band layout, a band's LIP in scan order and the scheduler's walk.
struct Coder {
    Band band[3][kMaxLevel][kBands];
    int16_t* data = nullptr;
    size_t width = 0, height = 0, levels = 0, planes = 0;
    int mode = 0, scan = 0, subsampling = 0;

    void layout()                                                   // SQZ_common_init_context :1805-1827 (level levels-1 is the finest)
    {
        for (size_t p = 0; p < planes; ++p) {
            size_t w = width, h = height;
            int16_t* base = data + p * w * h;
            for (int level = (int)levels - 1; level >= 0; --level) {
                for (size_t o = level > 0; o < (size_t)kBands; ++o) {
                    Band& b = band[p][level][o];
                    b.data = base;
                    b.width = (w + !(o & 1u)) >> 1; b.height = (h + !(o > 1u)) >> 1;
                    b.round = schedule(mode, (int)p, level, (int)o) + (subsampling & (int)(p > 0));
                    b.stride = width << (levels - (size_t)level);
                    if (o & 1u) b.data += (w + 1u) >> 1;
                    if (o > 1u) b.data += b.stride >> 1;
                }
                w = (w + 1u) >> 1; h = (h + 1u) >> 1;
            }
        }
    }
    bool init_lists(Band& b)                                        // SQZ_common_init_subband :1850-1864 with SQZ_scan_init :1124-1139
    {
        b.capacity = b.width * b.height; b.used = 0;
        free(b.nodes);
        b.nodes = static_cast<Node*>(calloc(b.capacity ? b.capacity : 1, sizeof(Node)));
        if (!b.nodes) return false;
        b.lip = b.lsp = b.nsp = List{};
        switch (scan) {
        case 0: for (size_t y = 0; y < b.height; ++y) for (size_t x = 0; x < b.width; ++x) b.add(b.lip, x, y); break;       // SQZ_scan_raster :797-808
        case 1: { Snake s(b.width, b.height, 4, 15); fill_lip(b, s); break; }
        case 2: { Morton s(b.width, b.height); fill_lip(b, s); break; }
        default: { Hilbert s(b.width, b.height); fill_lip(b, s); break; }
        }
        return true;
    }
    // SQZ_schedule_task :2105-2168.  task(band, first visit) > 0: go on; 0: the stream is at its end; < 0: give up, and that is the result
    template <class AtEnd, class Task> int walk(AtEnd at_end, Task task)
    {
        size_t state = 0, plane = 0, level = 0, o = 0;
        int round = 0; bool done = false;
        while (!done && !at_end()) {
            done = true;
            for (;;) {
                Band& b = band[plane][level][o];
                if (round < b.round || (round > b.round && b.bitplane == 0)) done = done && round > b.round;
                else {
                    const int r = task(b, b.round == round);
                    if (r <= 0) return r;
                    done = done && b.bitplane == 0;
                }
                if (!state) {                                       // plane 0 alone
                    if (++o >= (size_t)kBands) {
                        ++level;
                        o = level < levels;
                        if (o == 0u) { level = 0; state = plane = planes > 1u; if (!state) break; }
                    }
                } else if (++plane >= planes) {                     // planes 1.. per orientation
                    plane = 1;
                    if (++o >= (size_t)kBands) {
                        ++level;
                        o = level < levels;
                        if (o == 0u) { level = 0; state = plane = 0; break; }
                    }
                }
            }
            ++round;
        }
        return 0;
    }
};

struct Decoder : Coder {
    BitReader in;

    bool init_band(Band& b)                                         // SQZ_decode_init_subband :1890-1899
    {
        if (!init_lists(b)) return false;
        b.max_bitplane = in.bits(4);                                // -1 at the end of the buffer
        b.bitplane = b.max_bitplane;
        return true;
    }
    bool read_run(uint32_t* run)                                    // SQZ_decode_read_wdr_run :1941-1951
    {
        *run = 1u;
        while (in.bit() == 0) {
            const int b = in.bit();
            if (b < 0) return false;
            *run += *run + (uint32_t)b;                             // 32 unsigned bits: wraps
        }
        return true;
    }
    bool sorting_pass(Band& b)                                      // :1988-2020
    {
        if (b.lip.length == 0u || b.bitplane <= 0) return true;
        int32_t pixel = b.lip.head, prev = -1;
        const int16_t mask = (int16_t)(uint16_t)(1u << b.bitplane);
        for (;;) {
            uint32_t run;
            const int sign = in.bit();
            if (sign < 0 || !read_run(&run)) break;
            while (--run > 0u && pixel >= 0) { prev = pixel; pixel = b.nodes[pixel].next; }
            if (pixel < 0) break;
            b.at(pixel) = (int16_t)(b.at(pixel) | mask | sign);
            pixel = b.exchange(b.lip, b.nsp, pixel, prev);
        }
        return !in.at_end();
    }
    bool refinement_pass(Band& b)                                   // :2039-2057
    {
        const int16_t mask = (int16_t)(uint16_t)(1u << (b.bitplane & 31));      // (bitplane -1: the LSP is empty, the mask is not used)
        for (int32_t pixel = b.lsp.head; pixel >= 0; pixel = b.nodes[pixel].next) {
            const int v = in.bit();
            if (v > 0) b.at(pixel) = (int16_t)(b.at(pixel) | mask);
            else if (v < 0) break;
        }
        return !in.at_end();
    }
    bool bitplane(Band& b)                                          // SQZ_decode_bitplane :2070-2080
    {
        if (!sorting_pass(b) || !refinement_pass(b)) return false;
        b.merge(b.nsp, b.lsp);
        b.bitplane -= b.bitplane > 0;
        return !in.at_end();
    }
    bool run()                                                      // false = out of memory
    {
        return walk([&] { return in.at_end(); }, [&](Band& b, bool first) {
            if (first && !init_band(b)) return -1;
            return bitplane(b) ? 1 : 0;
        }) == 0;
    }
    void round_coefficients()                                       // :2082-2103
    {
        for (size_t p = 0; p < planes; ++p) for (size_t l = 0; l < levels; ++l) for (size_t o = l > 0; o < (size_t)kBands; ++o) {
            Band& b = band[p][l][o];
            if (b.max_bitplane == 0 || b.bitplane < 2) continue;
            const int16_t rm = (int16_t)(uint16_t)(((1u << b.bitplane) - 1u) ^ 1u);
            for (int32_t px = b.lsp.head; px >= 0; px = b.nodes[px].next) b.at(px) = (int16_t)(b.at(px) | rm);
        }
    }
};

// ---- the writer: SQZ_encode behind SQZ_dwt_convert_to_sign_magnitude (:2232-2237) ----
struct BitWriter {                                                  // SQZ_bit_buffer_t, write side :570-623
    uint8_t *data, *ptr, *eob; uint32_t index = 0;
    bool at_end() const { return ptr >= eob; }
    size_t bits_used() const { return (size_t)(ptr - data) * 8u + index; }
    bool bit(uint32_t b)
    {
        if (at_end()) return false;
        *ptr |= (uint8_t)(b << (7u - index));
        if (index < 7u) ++index; else { ++ptr; index = 0; }
        return true;
    }
    bool bits(uint32_t v, uint32_t width)                           // a width of 0 still fails at the end of the buffer (:599)
    {
        for (;;) {
            if (at_end()) return false;
            const uint32_t room = 8u - index;
            if (room >= width) {
                *ptr |= (uint8_t)((v & ((1u << width) - 1u)) << (room - width));
                index += width;
                if (index > 7u) { ++ptr; index = 0; }
                return true;
            }
            *ptr |= (uint8_t)((v >> (width - room)) & ((1u << room) - 1u));
            ++ptr; index = 0; width -= room;
        }
    }
};

uint32_t interleave(uint32_t i)                                     // :548-556
{
    i &= 0x0000FFFFu; i = (i ^ (i << 8)) & 0x00FF00FFu; i = (i ^ (i << 4)) & 0x0F0F0F0Fu;
    i = (i ^ (i << 2)) & 0x33333333u; i = (i ^ (i << 1)) & 0x55555555u;
    return i;
}

constexpr int kUndefinedShift = -2;                                 // Encoder::init_band

struct Encoder : Coder {
    BitWriter out;

    // SQZ_encode_init_subband :1866-1876.  SQZ_dwt_get_max compares SHORTS: a sign-magnitude value of 32768 or more (|coefficient| >=
    // 16384) is a negative short and never the maximum while the band holds one value that is not.  Then max >> 1 <= 16383, max_bitplane
    // <= 14 and everything below is defined; it is reproduced, blind to those values' top bit as the reference is.  A band of nothing but
    // such values has a negative maximum: SQZ_ilog2 of it as uint is 32, 1u << 32 is not defined -- the image is refused.
    int init_band(Band& b)
    {
        if (!init_lists(b)) return -1;
        int16_t max = *b.data;
        for (size_t y = 0; y < b.height; ++y) {
            const int16_t* row = b.data + y * b.stride;
            for (size_t x = 0; x < b.width; ++x) if (row[x] > max) max = row[x];
        }
        if (max < 0) return kUndefinedShift;
        b.max_bitplane = (int)ilog2((uint32_t)(max >> 1));
        b.bitplane = b.max_bitplane;
        out.bits((uint32_t)b.max_bitplane, 4u);
        return 1;
    }
    bool write_run(uint32_t run)                                    // SQZ_encode_write_wdr_run :1928-1939
    {
        const uint32_t cost = ilog2(run) - 1u;
        if (cost <= 16u) return out.bits(interleave(run), cost * 2u);
        return out.bits(interleave(run >> 16), (cost - 16u) * 2u) && out.bits(interleave(run), 32u);
    }
    bool sorting_pass(Band& b)                                      // :1953-1986
    {
        if (b.lip.length == 0u || b.bitplane <= 0) return true;
        int32_t pixel = b.lip.head, prev = -1;
        const int16_t mask = (int16_t)(uint16_t)(1u << b.bitplane);
        uint32_t i = 1u, last = 0u;
        while (pixel >= 0) {
            const int16_t v = b.at(pixel);
            if (v & mask) {
                if (!out.bits(2u | (uint32_t)(v & 1), 1u + (last != 0u)) || !write_run(i - last)) break;
                last = i;
                pixel = b.exchange(b.lip, b.nsp, pixel, prev);
            } else { prev = pixel; pixel = b.nodes[pixel].next; }
            ++i;
        }
        out.bits(3u, 1u + (b.nsp.length > 0u));                     // the WDR termination: a run past the LIP
        write_run(i - last);
        out.bit(1u);
        return !out.at_end();
    }
    bool refinement_pass(Band& b)                                   // :2022-2037
    {
        const int16_t mask = (int16_t)(uint16_t)(1u << b.bitplane);
        for (int32_t pixel = b.lsp.head; pixel >= 0; pixel = b.nodes[pixel].next)
            if (!out.bit((b.at(pixel) & mask) != 0)) break;
        return !out.at_end();
    }
    bool bitplane(Band& b)                                          // SQZ_encode_bitplane :2059-2068
    {
        if (!sorting_pass(b) || !refinement_pass(b)) return false;
        b.merge(b.nsp, b.lsp);
        b.bitplane -= b.bitplane > 0;
        return !out.at_end();
    }
    int run()                                                       // 0, -1 out of memory, kUndefinedShift
    {
        return walk([&] { return out.at_end(); }, [&](Band& b, bool first) {
            if (first) { const int r = init_band(b); if (r < 0) return r; }
            return bitplane(b) ? 1 : 0;
        });
    }
};

} // namespace

int sqz_fail(const char* why) { return set_error(GAMUT_HIP_ERR_DECODE, "sqz: %s", why); }

// Coder::layout with offsets in place of pointers, for the device writer (sqz_write.hip), which gathers the bands itself
void sqz_band_geometry(const gamut_hip_sqz_encode_desc& d, SqzBandGeom g[kSqzSlots])
{
    memset(g, 0, sizeof(SqzBandGeom) * kSqzSlots);
    const size_t planes = d.color_mode == 0 ? 1 : 3, levels = (size_t)d.levels, width = (size_t)d.width;
    for (size_t p = 0; p < planes; ++p) {
        size_t w = width, h = (size_t)d.height;
        const size_t base = p * w * h;
        for (int level = (int)levels - 1; level >= 0; --level) {
            for (size_t o = level > 0; o < (size_t)kBands; ++o) {
                SqzBandGeom& b = g[(p * kMaxLevel + (size_t)level) * kBands + o];
                b.width = (uint32_t)((w + !(o & 1u)) >> 1); b.height = (uint32_t)((h + !(o > 1u)) >> 1);
                b.round = schedule(d.color_mode, (int)p, level, (int)o) + ((d.subsampling != 0) & (int)(p > 0));
                b.stride = (uint32_t)(width << (levels - (size_t)level));
                size_t off = base;
                if (o & 1u) off += (w + 1u) >> 1;
                if (o > 1u) off += b.stride >> 1;
                b.offset = (int64_t)off;
            }
            w = (w + 1u) >> 1; h = (h + 1u) >> 1;
        }
    }
}

// a band's LIP as init_lists fills it, as (x, y) pairs
int sqz_scan_order(int order, int width, int height, uint16_t* xy)
{
    if (order < 0 || order > 3 || width < 1 || height < 1 || width > 65535 || height > 65535 || !xy)
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_scan_order: order %d, %d x %d", order, width, height);
    const size_t w = (size_t)width, h = (size_t)height, n = w * h;
    size_t k = 0;
    auto put = [&](size_t x, size_t y) { if (k < n) { xy[2 * k] = (uint16_t)x; xy[2 * k + 1] = (uint16_t)y; } ++k; };      // Band::add's capacity guard
    switch (order) {
    case 0: for (size_t y = 0; y < h; ++y) for (size_t x = 0; x < w; ++x) put(x, y); break;
    case 1: { Snake s(w, h, 4, 15); do put(s.x, s.y); while (s.next()); break; }
    case 2: { Morton s(w, h); do put(s.x, s.y); while (s.next()); break; }
    default: { Hilbert s(w, h); do put(s.x, s.y); while (s.next()); break; }
    }
    if (k != n) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_scan_order: scan %d visits %zu positions of a %d x %d band", order, k, width, height);
    return GAMUT_HIP_OK;
}

int sqz_undefined_shift_error()
{
    return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: a subband holds nothing but coefficients of magnitude 16384 and more; the reference's bit plane for it is 1u << 32");
}

// SQZ_validate_input :2170-2197, read-only mode
bool sqz_valid_geometry(int64_t w, int64_t h, int mode, int scan, int levels)
{
    if (w < 8 || w > 65535 || h < 8 || h > 65535 || mode < 0 || mode > 3 || scan < 0 || scan > 3 || levels < 1 || levels > kMaxLevel) return false;
    uint32_t max_level = ilog2((uint32_t)(w > h ? h : w)) - 3u;
    if (max_level > (uint32_t)kMaxLevel) max_level = kMaxLevel;
    return (uint32_t)levels <= max_level;
}

// SQZ_decode_header :1913-1926 + SQZ_validate_input; the bit stream goes on at byte 6
int sqz_parse_header(const uint8_t* data, size_t len, gamut_hip_sqz_info* info)
{
    memset(info, 0, sizeof(*info));
    if (!data) len = 0;
    info->detected = len >= 1 && data[0] == 0xA5;                   // detectSQZ plugins/sqz.d:135-139
    BitReader in{ data, data + len };
    if (in.bits(8) != 0xA5) return sqz_fail("wrong magic byte");
    const int w = in.bits(16), h = in.bits(16), mode = in.bits(2), lv = in.bits(3), scan = in.bits(2), ss = in.bit();
    if (ss < 0 || in.at_end()) return sqz_fail("no bit stream behind the 6-byte header");
    if (!sqz_valid_geometry((int64_t)w + 1, (int64_t)h + 1, mode, scan, lv + 1)) return sqz_fail("corrupted header (side below 8 or too many levels for the size)");
    info->width = w + 1; info->height = h + 1; info->color_mode = mode; info->levels = lv + 1; info->scan_order = scan; info->subsampling = ss;
    info->planes = mode == 0 ? 1 : 3;
    info->pixel_type = mode == 0 ? 0 : 9;                           // PixelType.l8 / rgb8 (plugins/sqz.d:100-103)
    return GAMUT_HIP_OK;
}

int sqz_decode_coeffs(const uint8_t* data, size_t len, int16_t* out, size_t capacity, gamut_hip_sqz_info* info)
{
    if (int rc = sqz_parse_header(data, len, info)) return rc;
    const size_t n = (size_t)info->width * (size_t)info->height * (size_t)info->planes;
    if (capacity < n) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_decode_coeffs: capacity %zu below planes * width * height = %zu", capacity, n);
    std::unique_ptr<Decoder> d(new (std::nothrow) Decoder());
    if (!d) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz: out of host memory");
    memset(out, 0, n * sizeof(int16_t));                            // calloc :1800
    d->in = BitReader{ data + 6, data + len };
    d->data = out;
    d->width = (size_t)info->width; d->height = (size_t)info->height; d->levels = (size_t)info->levels; d->planes = (size_t)info->planes;
    d->mode = info->color_mode; d->scan = info->scan_order; d->subsampling = info->subsampling;
    d->layout();
    if (!d->run()) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz: out of host memory for a subband's lists");
    d->round_coefficients();
    return GAMUT_HIP_OK;
}

// SQZ_validate_input :2170-2197 with read_only = 0: too many levels are CLAMPED to what the size admits, everything else is refused
int sqz_encode_check(gamut_hip_sqz_encode_desc* d)
{
    if (d->width < 8 || d->width > 65535 || d->height < 8 || d->height > 65535 || d->color_mode < 0 || d->color_mode > 3 || d->scan_order < 0 ||
        d->scan_order > 3 || d->levels < 1 || d->levels > kMaxLevel)
        return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: %d x %d, colour mode %d, scan order %d, %d levels cannot be encoded (sides 8..65535, modes and scans 0..3, levels 1..8)",
                         d->width, d->height, d->color_mode, d->scan_order, d->levels);
    uint32_t max_level = ilog2((uint32_t)(d->width > d->height ? d->height : d->width)) - 3u;
    if (max_level > (uint32_t)kMaxLevel) max_level = kMaxLevel;
    if ((uint32_t)d->levels > max_level) d->levels = (int32_t)max_level;
    return GAMUT_HIP_OK;
}

// SQZ_encode :2216-2237 without the colour stage and the DWT: `d` has passed sqz_encode_check, planes is the sign-magnitude buffer
int sqz_encode_coeffs(const int16_t* planes, const gamut_hip_sqz_encode_desc& d, uint8_t* dst, int64_t* len)
{
    *len = 0;
    if (d.budget <= 6) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: a budget of %lld bytes does not hold the 6-byte header and one more bit", (long long)d.budget);
    std::unique_ptr<Encoder> e(new (std::nothrow) Encoder());
    if (!e) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz: out of host memory");
    memset(dst, 0, (size_t)d.budget);                               // saveSQZ plugins/sqz.d:167-169: the writer only ORs bits in
    e->out = BitWriter{ dst, dst, dst + d.budget };
    BitWriter& out = e->out;                                        // SQZ_encode_header :1901-1911
    out.bits(0xA5u, 8u); out.bits((uint32_t)(d.width - 1), 16u); out.bits((uint32_t)(d.height - 1), 16u); out.bits((uint32_t)d.color_mode, 2u);
    out.bits((uint32_t)(d.levels - 1), 3u); out.bits((uint32_t)d.scan_order, 2u); out.bit(d.subsampling != 0);
    if (out.at_end()) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz: no room behind the header");      // (budget > 6: not reached)
    e->data = const_cast<int16_t*>(planes);                         // the writer only reads them
    e->width = (size_t)d.width; e->height = (size_t)d.height; e->levels = (size_t)d.levels; e->planes = d.color_mode == 0 ? 1 : 3;
    e->mode = d.color_mode; e->scan = d.scan_order; e->subsampling = d.subsampling != 0;
    e->layout();
    const int r = e->run();
    if (r == kUndefinedShift) return sqz_undefined_shift_error();
    if (r < 0) return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz: out of host memory for a subband's lists");
    *len = (int64_t)((out.bits_used() + 7u) / 8u);
    return GAMUT_HIP_OK;
}

// The two sRGB tables of the colour stage (SQZ_sRGB_to_linear :1251-1285, SQZ_linear_to_sRGB :1287-1321) are the sRGB transfer
// functions sampled at i / 255 and i / 511, rounded to nearest: the formulas reproduce every entry (tests/test_sqz_cpu.py pins the
// SHA-256 of both).  The second decodes, the first encodes.
const uint16_t* sqz_srgb_to_linear_table()
{
    static uint16_t t[256];
    static const bool once = [] {
        for (int i = 0; i < 256; ++i) {
            double v = i / 255.0;
            v = v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4);
            t[i] = (uint16_t)floor(65535.0 * v + 0.5);
        }
        return true;
    }();
    (void)once;
    return t;
}
const uint8_t* sqz_linear_to_srgb_table()
{
    static uint8_t t[512];
    static const bool once = [] {
        for (int i = 0; i < 512; ++i) {
            double v = i / 511.0;
            v = v <= 0.0031308 ? 12.92 * v : 1.055 * pow(v, 1.0 / 2.4) - 0.055;
            t[i] = (uint8_t)floor(255.0 * v + 0.5);
        }
        return true;
    }();
    (void)once;
    return t;
}

} // namespace gamut

using namespace gamut;

extern "C" {

int gamut_hip_sqz_read_header(const uint8_t* data, size_t len, gamut_hip_sqz_info* info)
{
    clear_error();
    if (!info) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_read_header: info is NULL");
    return sqz_parse_header(data, len, info);
}

int gamut_hip_sqz_decode_coeffs(const uint8_t* data, size_t len, int16_t* planes, size_t capacity, gamut_hip_sqz_info* info)
{
    clear_error();
    gamut_hip_sqz_info own;
    if (!planes && capacity) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_decode_coeffs: planes is NULL");
    try {
        return sqz_decode_coeffs(data, len, planes, planes ? capacity : 0, info ? info : &own);
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_decode_coeffs: out of host memory");
    }
}

const uint8_t* gamut_hip_sqz_linear_to_srgb_table(void) { return sqz_linear_to_srgb_table(); }

int64_t gamut_hip_sqz_budget_from_flags(int width, int height, int flags)                  // saveSQZ plugins/sqz.d:153-158
{
    int bpp8 = (flags >> 5) & 0xff;
    if (bpp8 == 0) bpp8 = 0x50;
    const double bpp = (double)((float)bpp8 / 32.0f);
    return 6 + (int64_t)((double)width * height * bpp / 8.0);
}

int gamut_hip_sqz_scan_order(int order, int width, int height, uint16_t* xy)
{
    clear_error();
    try {
        return sqz_scan_order(order, width, height, xy);
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_scan_order: out of host memory");
    }
}

int gamut_hip_sqz_encode_coeffs(const int16_t* planes, const gamut_hip_sqz_encode_desc* desc, uint8_t* dst, int64_t* len)
{
    clear_error();
    if (len) *len = 0;
    if (!planes || !desc || !dst || !len) return set_error(GAMUT_HIP_ERR_INVALID_ARG, "sqz_encode_coeffs: NULL argument");
    gamut_hip_sqz_encode_desc d = *desc;
    if (int rc = sqz_encode_check(&d)) return rc;
    try {
        return sqz_encode_coeffs(planes, d, dst, len);
    } catch (...) {
        return set_error(GAMUT_HIP_ERR_OUT_OF_MEMORY, "sqz_encode_coeffs: out of host memory");
    }
}

} // extern "C"
