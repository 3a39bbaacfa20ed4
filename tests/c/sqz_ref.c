/* sqz_ref.c -- SQZ_decode and SQZ_encode of the reference (source/gamut/codecs/sqz.d) restated serially in C for the tests.
 *
 * The decoder is split where the library splits it: sqzref_coeffs() is SQZ_decode up to and including
 * SQZ_decode_round_coefficients (sign-magnitude coefficients, low bit = sign), sqzref_pixels() is the rest (two's complement,
 * the 5/3 integer IDWT level by level the way the reference interleaves rows, the colour transform).  sqzref_encode() makes
 * test files: every colour mode, scan order, level count, subsampling flag and byte budget.
 *
 * The two sRGB tables are generated from the sRGB transfer functions; tests/test_sqz_cpu.py pins their SHA-256.
 * Arithmetic that the reference does in `short` wraps here through explicit casts; `>>` of negative values is arithmetic
 * (checked by sqzref_selftest). */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

typedef int16_t coef_t;
enum { MAX_LEVEL = 8, BANDS = 4, MIN_DIM = 8, MAX_DIM = 65535, MAGIC = 0xA5 };

/* ---- bit buffer ---- */
typedef struct { uint8_t *data, *ptr, *eob; unsigned index; } bitbuf_t;
static void bb_init(bitbuf_t* b, void* p, size_t n) { b->data = b->ptr = (uint8_t*)p; b->eob = b->data + n; b->index = 0; }
static int bb_eob(const bitbuf_t* b) { return b->ptr >= b->eob; }
static int bb_read_bit(bitbuf_t* b)
{
    if (bb_eob(b)) return -1;
    int bit = (*b->ptr >> (7 - b->index)) & 1;
    if (b->index < 7) b->index++; else { b->ptr++; b->index = 0; }
    return bit;
}
static int bb_read_bits(bitbuf_t* b, unsigned width)
{
    int bits = 0;
    for (;;) {
        if (bb_eob(b)) return -1;
        unsigned avail = 8u - b->index;
        if (avail >= width) {
            bits = (int)((unsigned)bits << width);
            bits |= (*b->ptr >> (avail - width)) & ((1u << width) - 1u);
            b->index += width;
            if (b->index > 7) { b->ptr++; b->index = 0; }
            break;
        }
        bits = (int)((unsigned)bits << avail);
        bits |= *b->ptr & ((1u << avail) - 1u);
        b->ptr++; b->index = 0; width -= avail;
    }
    return bits;
}
static int bb_write_bit(bitbuf_t* b, unsigned bit)
{
    if (bb_eob(b)) return 0;
    *b->ptr |= (uint8_t)(bit << (7 - b->index));
    if (b->index < 7) b->index++; else { b->ptr++; b->index = 0; }
    return 1;
}
static int bb_write_bits(bitbuf_t* b, unsigned bits, unsigned width)
{
    for (;;) {
        if (bb_eob(b)) return 0;
        unsigned room = 8u - b->index;
        if (room >= width) {
            unsigned m = width >= 32 ? 0xFFFFFFFFu : (1u << width) - 1u;
            *b->ptr |= (uint8_t)((bits & m) << (room - width));
            b->index += width;
            if (b->index > 7) { b->ptr++; b->index = 0; }
            return 1;
        }
        *b->ptr |= (uint8_t)((bits >> (width - room)) & ((1u << room) - 1u));
        b->ptr++; b->index = 0; width -= room;
    }
}

/* ---- lists: nodes in one cache per subband, linked by index ---- */
typedef struct { uint16_t x, y; int next; } node_t;
typedef struct { int head, tail; size_t length; } list_t;              /* -1 = null */
typedef struct {
    node_t* nodes; size_t capacity, index;
    list_t LIP, LSP, NSP;
    coef_t* data; size_t width, height, stride;
    int max_bitplane, bitplane, round;
} band_t;
typedef struct {
    band_t band[3][MAX_LEVEL][BANDS];
    coef_t* plane[3];
    coef_t* data;
    bitbuf_t buf;
    int mode, scan; size_t width, height, levels, planes; int subsampling;
} ctx_t;

static void list_add(band_t* b, list_t* l, unsigned x, unsigned y)
{
    if (b->index >= b->capacity) return;
    int k = (int)b->index;
    if (l->head < 0) l->head = k; else if (l->tail >= 0) b->nodes[l->tail].next = k;
    l->tail = k; l->length++;
    b->nodes[k].x = (uint16_t)x; b->nodes[k].y = (uint16_t)y; b->nodes[k].next = -1;
    b->index++;
}
static int list_exchange(band_t* b, list_t* src, list_t* dst, int node, int prev)
{
    int next = b->nodes[node].next;
    if (prev >= 0) b->nodes[prev].next = next; else src->head = next;
    src->length--;
    if (dst->head < 0) dst->head = node; else if (dst->tail >= 0) b->nodes[dst->tail].next = node;
    dst->tail = node; dst->length++;
    b->nodes[node].next = -1;
    return next;
}
static void list_merge(band_t* b, list_t* src, list_t* dst)
{
    if (src->head < 0) return;
    if (dst->tail >= 0) b->nodes[dst->tail].next = src->head; else dst->head = src->head;
    dst->tail = src->tail; dst->length += src->length;
    src->length = 0; src->head = src->tail = -1;
}

/* ---- helpers ---- */
static unsigned ilog2u(unsigned x) { unsigned n = 0; while (x) { ++n; x >>= 1; } return n; }       /* bsr + 1, 0 for 0 */
static unsigned mirror(int v, int maximum)
{
    if (maximum == 0) return 0;
    while ((unsigned)v > (unsigned)maximum) { v = -v; if (v < 0) v += 2 * maximum; }
    return (unsigned)v;
}
static unsigned deinterleave(unsigned i)
{
    i &= 0x55555555u; i = (i ^ (i >> 1)) & 0x33333333u; i = (i ^ (i >> 2)) & 0x0F0F0F0Fu;
    i = (i ^ (i >> 4)) & 0x00FF00FFu; i = (i ^ (i >> 8)) & 0x0000FFFFu; return i;
}
static unsigned interleave(unsigned i)
{
    i &= 0xFFFFu; i = (i ^ (i << 8)) & 0x00FF00FFu; i = (i ^ (i << 4)) & 0x0F0F0F0Fu;
    i = (i ^ (i << 2)) & 0x33333333u; i = (i ^ (i << 1)) & 0x55555555u; return i;
}
static int iabs(int x) { return x < 0 ? -x : x; }
static int isign(int x) { return x < 0 ? -1 : x > 0 ? 1 : 0; }

/* ---- scan orders: fill the LIP of a w x h subband ---- */
static void scan_raster(band_t* b)
{
    for (size_t y = 0; y < b->height; ++y) for (size_t x = 0; x < b->width; ++x) list_add(b, &b->LIP, (unsigned)x, (unsigned)y);
}
static void scan_snake(band_t* b)
{
    size_t width = b->width, height = b->height, tw = 4, th = 15;
    if (tw > width) tw = width;
    if (th > height) th = height;
    size_t grid_w, grid_h, col_rem, row_rem;
    int step = 1;
    for (;;) {                                                       /* an odd number of grid columns */
        grid_w = (width + tw - 1) / tw;
        if (grid_w & 1) break;
        tw += (size_t)(long)step;
        if (tw > width) tw = width; else if (tw == 0) tw = 1;
        step = -(iabs(step) + 1) * ((step > 0) - (step < 0));
    }
    col_rem = width % tw; if (col_rem == 0) col_rem = tw;
    step = 2;
    for (;;) {                                                       /* an odd number of rows in the last grid row's tiles */
        row_rem = height % th;
        if (row_rem > 0 && !(row_rem & 1)) {
            th += (size_t)(long)step;
            if (th > height) th = height; else if (th == 0) th = 1;
            step = -(iabs(step) + 2) * ((step > 0) - (step < 0));
        } else { if (row_rem == 0) row_rem = th; break; }
    }
    grid_h = (height + th - 1) / th;
    /* the walk of SQZ_scan_snake, as nested loops */
    for (size_t gy = 0; gy < grid_h; ++gy) {
        /* the FIRST grid row starts with tile.height = th even when the grid has one row only (init: grid.height > 1 || rows.remaining > 0) */
        size_t tile_h = gy == 0 ? th : (gy < grid_h - 1 ? th : row_rem);
        size_t off_y = gy * th;
        int rows_odd = (int)(gy & 1);
        for (size_t ci = 0; ci < grid_w; ++ci) {
            size_t gx, tile_w;
            int col_odd;
            if (gy == 0 && ci == 0) { gx = 0; col_odd = 0; tile_w = tw; }                  /* as initialised: tile.width = tile_width */
            else { gx = rows_odd ? (grid_w - 1) - ci : ci; col_odd = (int)(gx & 1); tile_w = gx < grid_w - 1 ? tw : col_rem; }
            size_t off_x = gx * tw;
            for (size_t ty = 0; ty < tile_h; ++ty) {
                size_t row = col_odd ? (tile_h - 1) - ty : ty;
                int r2l = (gy == 0 && ci == 0 && ty == 0) ? 0 : (int)((gy ^ row) & 1);
                for (size_t tx = 0; tx < tile_w; ++tx) {
                    size_t x = (r2l ? (tile_w - 1) - tx : tx) + off_x, y = row + off_y;
                    list_add(b, &b->LIP, (unsigned)x, (unsigned)y);
                }
            }
        }
    }
}
static void scan_morton(band_t* b)
{
    size_t width = b->width, height = b->height;
    size_t range = ilog2u((unsigned)(width > height ? height : width) - 1u);
    size_t mask = (size_t)((1ull << (range * 2u)) - 1u);
    size_t length = (size_t)(1ull << (range + ilog2u((unsigned)(width > height ? width : height) - 1u)));
    size_t index = 0;
    list_add(b, &b->LIP, 0, 0);
    for (;;) {
        int found = 0; size_t x = 0, y = 0;
        do {
            index++;
            x = deinterleave((unsigned)(index & mask));
            y = deinterleave((unsigned)((index >> 1) & mask));
            unsigned m = (unsigned)((index & ~mask) >> range);
            if (width > height) x |= m; else y |= m;
            if (x < width && y < height) { found = 1; break; }
        } while (index < length);
        if (!found) break;
        list_add(b, &b->LIP, (unsigned)x, (unsigned)y);
    }
}
typedef struct { int x, y, ax, ay, bx, by; } hitem_t;
static void scan_hilbert(band_t* b)
{
    hitem_t st[32]; int sp = 0;
    int width = (int)b->width, height = (int)b->height;
    if (width >= height) st[sp++] = (hitem_t){ 0, 0, width, 0, 0, height }; else st[sp++] = (hitem_t){ 0, 0, 0, height, width, 0 };
    while (sp > 0) {
        hitem_t cur = st[--sp];
        int w = iabs(cur.ax + cur.ay), h = iabs(cur.bx + cur.by);
        int dax = isign(cur.ax), day = isign(cur.ay), dbx = isign(cur.bx), dby = isign(cur.by);
        if (h == 1) { for (int i = 0; i < w; ++i) { list_add(b, &b->LIP, (unsigned)cur.x, (unsigned)cur.y); cur.x += dax; cur.y += day; } continue; }
        if (w == 1) { for (int i = 0; i < h; ++i) { list_add(b, &b->LIP, (unsigned)cur.x, (unsigned)cur.y); cur.x += dbx; cur.y += dby; } continue; }
        int ax2 = cur.ax / 2, ay2 = cur.ay / 2, bx2 = cur.bx / 2, by2 = cur.by / 2;
        int w2 = iabs(ax2 + ay2), h2 = iabs(bx2 + by2);
        if (2 * w > 3 * h) {
            if ((w2 % 2) != 0 && w > 2) { ax2 += dax; ay2 += day; }
            st[sp++] = (hitem_t){ cur.x + ax2, cur.y + ay2, cur.ax - ax2, cur.ay - ay2, cur.bx, cur.by };
            st[sp++] = (hitem_t){ cur.x, cur.y, ax2, ay2, cur.bx, cur.by };
        } else {
            if ((h2 % 2) != 0 && h > 2) { bx2 += dbx; by2 += dby; }
            st[sp++] = (hitem_t){ cur.x + (cur.ax - dax) + (bx2 - dbx), cur.y + (cur.ay - day) + (by2 - dby), -bx2, -by2, -(cur.ax - ax2), -(cur.ay - ay2) };
            st[sp++] = (hitem_t){ cur.x + bx2, cur.y + by2, cur.ax, cur.ay, cur.bx - bx2, cur.by - by2 };
            st[sp++] = (hitem_t){ cur.x, cur.y, bx2, by2, ax2, ay2 };
        }
    }
}
static int init_subband(ctx_t* c, band_t* b)
{
    b->capacity = b->width * b->height; b->index = 0;
    b->nodes = (node_t*)calloc(b->capacity, sizeof(node_t));
    if (!b->nodes) return -1;
    b->LIP = b->LSP = b->NSP = (list_t){ -1, -1, 0 };
    switch (c->scan) {
    case 0: scan_raster(b); break;
    case 1: scan_snake(b); break;
    case 2: scan_morton(b); break;
    default: scan_hilbert(b); break;
    }
    return 0;
}

/* ---- context ---- */
static const uint8_t kPlanes[4] = { 1, 3, 3, 3 };
static int schedule(int mode, int plane, int level, int o)
{
    static const uint8_t first[4] = { 0, 1, 1, 2 };
    if (plane == 0 || mode == 0) return plane == 0 ? (o == 0 ? 0 : first[o] + level) : 0;
    if (level == 0) return first[o] + 1;
    return o == 0 ? 0 : first[o] + level + 1;
}
static int init_context(ctx_t* c)
{
    c->data = (coef_t*)calloc(c->width * c->height * c->planes, sizeof(coef_t));
    if (!c->data) return -1;
    for (size_t p = 0; p < c->planes; ++p) {
        size_t w = c->width, h = c->height;
        c->plane[p] = c->data + p * w * h;
        for (int level = (int)c->levels - 1; level >= 0; --level) {
            for (size_t o = level > 0; o < BANDS; ++o) {
                band_t* b = &c->band[p][level][o];
                b->data = c->plane[p];
                b->width = (w + !(o & 1u)) >> 1; b->height = (h + !(o > 1u)) >> 1;
                b->round = schedule(c->mode, (int)p, level, (int)o) + (c->subsampling & (p > 0));
                b->stride = c->width << (c->levels - (size_t)level);
                if (o & 1u) b->data += (w + 1) >> 1;
                if (o > 1u) b->data += b->stride >> 1;
            }
            w = (w + 1) >> 1; h = (h + 1) >> 1;
        }
    }
    return 0;
}
static void free_context(ctx_t* c)
{
    free(c->data);
    for (int p = 0; p < 3; ++p) for (int l = 0; l < MAX_LEVEL; ++l) for (int o = 0; o < BANDS; ++o) free(c->band[p][l][o].nodes);
}

/* ---- decoder passes ---- */
static int read_wdr_run(bitbuf_t* buf, uint32_t* run)
{
    *run = 1u;
    while (bb_read_bit(buf) == 0) {
        int bit = bb_read_bit(buf);
        if (bit < 0) return 0;
        *run += *run + (uint32_t)bit;
    }
    return 1;
}
static int dec_sorting(band_t* b, bitbuf_t* buf)
{
    if (b->LIP.length == 0 || b->bitplane <= 0) return 1;
    int pixel = b->LIP.head, prev = -1;
    coef_t mask = (coef_t)(1u << b->bitplane);
    for (;;) {
        uint32_t run;
        int sign = bb_read_bit(buf);
        if (sign < 0 || !read_wdr_run(buf, &run)) break;
        while (--run > 0 && pixel >= 0) { prev = pixel; pixel = b->nodes[pixel].next; }
        if (pixel < 0) break;
        b->data[b->nodes[pixel].y * b->stride + b->nodes[pixel].x] |= (coef_t)(mask | sign);
        pixel = list_exchange(b, &b->LIP, &b->NSP, pixel, prev);
    }
    return !bb_eob(buf);
}
static int dec_refinement(band_t* b, bitbuf_t* buf)
{
    coef_t mask = (coef_t)(1u << (b->bitplane & 31));                 /* (bitplane is -1 when the 4 bits were missing: the LSP is empty then) */
    for (int pixel = b->LSP.head; pixel >= 0; pixel = b->nodes[pixel].next) {
        int v = bb_read_bit(buf);
        if (v > 0) b->data[b->nodes[pixel].y * b->stride + b->nodes[pixel].x] |= mask;
        else if (v < 0) break;
    }
    return !bb_eob(buf);
}
static int dec_bitplane(ctx_t* c, band_t* b, int first)
{
    bitbuf_t* buf = &c->buf;
    if (first) {
        if (init_subband(c, b)) return -1;
        b->max_bitplane = bb_read_bits(buf, 4);
        b->bitplane = b->max_bitplane;
    }
    if (!dec_sorting(b, buf) || !dec_refinement(b, buf)) return 0;
    list_merge(b, &b->NSP, &b->LSP);
    b->bitplane -= b->bitplane > 0;
    return !bb_eob(buf);
}

/* ---- encoder passes ---- */
static int write_wdr_run(bitbuf_t* buf, uint32_t run)
{
    unsigned cost = ilog2u(run) - 1u;
    if (cost <= 16u) return bb_write_bits(buf, interleave(run), cost * 2u);
    return bb_write_bits(buf, interleave(run >> 16), (cost - 16) * 2u) && bb_write_bits(buf, interleave(run), 32u);
}
static int enc_sorting(band_t* b, bitbuf_t* buf)
{
    if (b->LIP.length == 0 || b->bitplane <= 0) return 1;
    int pixel = b->LIP.head, prev = -1;
    coef_t mask = (coef_t)(1u << b->bitplane);
    uint32_t i = 1, last = 0;
    while (pixel >= 0) {
        coef_t v = b->data[b->nodes[pixel].y * b->stride + b->nodes[pixel].x];
        if (v & mask) {
            if (!bb_write_bits(buf, 2u | (unsigned)(v & 1), 1u + !!last) || !write_wdr_run(buf, i - last)) break;
            last = i;
            pixel = list_exchange(b, &b->LIP, &b->NSP, pixel, prev);
        } else { prev = pixel; pixel = b->nodes[pixel].next; }
        ++i;
    }
    bb_write_bits(buf, 3u, 1u + (b->NSP.length > 0));
    write_wdr_run(buf, i - last);
    bb_write_bit(buf, 1u);
    return !bb_eob(buf);
}
static int enc_refinement(band_t* b, bitbuf_t* buf)
{
    coef_t mask = (coef_t)(1u << b->bitplane);
    for (int pixel = b->LSP.head; pixel >= 0; pixel = b->nodes[pixel].next) {
        coef_t v = b->data[b->nodes[pixel].y * b->stride + b->nodes[pixel].x];
        if (!bb_write_bit(buf, !!(v & mask))) break;
    }
    return !bb_eob(buf);
}
static int enc_bitplane(ctx_t* c, band_t* b, int first)
{
    bitbuf_t* buf = &c->buf;
    if (first) {
        if (init_subband(c, b)) return -1;
        coef_t max = *b->data;
        for (size_t y = 0; y < b->height; ++y) for (size_t x = 0; x < b->width; ++x) if (b->data[y * b->stride + x] > max) max = b->data[y * b->stride + x];
        b->max_bitplane = (int)ilog2u((unsigned)(int)(max >> 1));
        b->bitplane = b->max_bitplane;
        bb_write_bits(buf, (unsigned)b->max_bitplane, 4u);
    }
    if (!enc_sorting(b, buf) || !enc_refinement(b, buf)) return 0;
    list_merge(b, &b->NSP, &b->LSP);
    b->bitplane -= b->bitplane > 0;
    return !bb_eob(buf);
}

/* ---- SQZ_schedule_task ---- */
static int run_schedule(ctx_t* c, int (*task)(ctx_t*, band_t*, int))
{
    size_t state = 0, plane = 0, level = 0, o = 0;
    int round = 0, done = 0;
    while (!done && !bb_eob(&c->buf)) {
        done = 1;
        for (;;) {
            band_t* b = &c->band[plane][level][o];
            if (round < b->round || (round > b->round && b->bitplane == 0)) done &= round > b->round;
            else {
                int r = task(c, b, b->round == round);
                if (r < 0) return -1;
                if (!r) return 0;
                done &= b->bitplane == 0;
            }
            if (!state) {
                if (++o >= BANDS) {
                    ++level;
                    o = level < c->levels;
                    if (o == 0) { level = 0; state = plane = c->planes > 1; if (!state) break; }
                }
            } else {
                if (++plane >= c->planes) {
                    plane = 1;
                    if (++o >= BANDS) {
                        ++level;
                        o = level < c->levels;
                        if (o == 0) { level = 0; state = plane = 0; break; }
                    }
                }
            }
        }
        ++round;
    }
    return 0;
}

/* ---- header ---- */
static int validate(size_t w, size_t h, int mode, int scan, size_t levels)
{
    if (w < MIN_DIM || w > MAX_DIM || h < MIN_DIM || h > MAX_DIM || mode < 0 || mode > 3 || scan < 0 || scan > 3 || levels == 0 || levels > MAX_LEVEL) return 0;
    unsigned max_level = ilog2u((unsigned)(w > h ? h : w)) - 3u;
    if (max_level > MAX_LEVEL) max_level = MAX_LEVEL;
    return levels <= max_level;
}
static int read_header(ctx_t* c)
{
    bitbuf_t* b = &c->buf;
    if (bb_read_bits(b, 8) != MAGIC) return 0;
    int w = bb_read_bits(b, 16), h = bb_read_bits(b, 16), mode = bb_read_bits(b, 2), lv = bb_read_bits(b, 3), scan = bb_read_bits(b, 2), ss = bb_read_bit(b);
    if (ss < 0 || bb_eob(b)) return 0;                                /* (a field of -1 is never used: the reference's verdict is !eob) */
    c->width = (size_t)w + 1; c->height = (size_t)h + 1; c->mode = mode; c->levels = (size_t)lv + 1; c->scan = scan; c->subsampling = !!ss;
    c->planes = kPlanes[mode];
    return validate(c->width, c->height, c->mode, c->scan, c->levels);
}

/* info[9]: width, height, planes, colour mode, levels, scan order, subsampling, pixel type (0 = l8, 9 = rgb8), detected.  0 = accepted */
long sqzref_header(const uint8_t* data, long len, int32_t* info)
{
    ctx_t* c = (ctx_t*)calloc(1, sizeof(ctx_t));
    if (!c) return -1;
    memset(info, 0, 9 * sizeof(int32_t));
    info[8] = len > 0 && data[0] == MAGIC;
    bb_init(&c->buf, (void*)data, (size_t)len);
    int ok = read_header(c);
    if (ok) {
        info[0] = (int32_t)c->width; info[1] = (int32_t)c->height; info[2] = (int32_t)c->planes; info[3] = c->mode; info[4] = (int32_t)c->levels;
        info[5] = c->scan; info[6] = c->subsampling; info[7] = c->planes == 1 ? 0 : 9;
    }
    free(c);
    return ok ? 0 : 1;
}

/* the coefficient stage: planes * w * h sign-magnitude coefficients.  0 = ok, 1 = refused, -1 = no memory / capacity */
long sqzref_coeffs(const uint8_t* data, long len, int16_t* out, long capacity)
{
    ctx_t* c = (ctx_t*)calloc(1, sizeof(ctx_t));
    if (!c) return -1;
    long rc = 1;
    bb_init(&c->buf, (void*)data, (size_t)len);
    if (read_header(c)) {
        size_t n = c->width * c->height * c->planes;
        if ((size_t)capacity < n || init_context(c)) rc = -1;
        else if (run_schedule(c, dec_bitplane) < 0) rc = -1;
        else {
            for (size_t p = 0; p < c->planes; ++p) for (size_t l = 0; l < c->levels; ++l) for (size_t o = l > 0; o < BANDS; ++o) {
                band_t* b = &c->band[p][l][o];
                if (b->max_bitplane == 0 || b->bitplane < 2) continue;
                coef_t rm = (coef_t)(((1u << b->bitplane) - 1u) ^ 1u);
                for (int px = b->LSP.head; px >= 0; px = b->nodes[px].next) b->data[b->nodes[px].y * b->stride + b->nodes[px].x] |= rm;
            }
            memcpy(out, c->data, n * sizeof(coef_t));
            rc = 0;
        }
    }
    free_context(c);
    free(c);
    return rc;
}

/* ---- tables ---- */
static uint16_t s2l[256];
static uint8_t l2s[512];
static int tables_ready;
static void tables(void)
{
    if (tables_ready) return;
    for (int i = 0; i < 256; ++i) { double v = i / 255.0; v = v <= 0.04045 ? v / 12.92 : pow((v + 0.055) / 1.055, 2.4); s2l[i] = (uint16_t)floor(65535.0 * v + 0.5); }
    for (int i = 0; i < 512; ++i) { double v = i / 511.0; v = v <= 0.0031308 ? 12.92 * v : 1.055 * pow(v, 1.0 / 2.4) - 0.055; l2s[i] = (uint8_t)floor(255.0 * v + 0.5); }
    tables_ready = 1;
}
void sqzref_tables(uint16_t* srgb_to_linear, uint8_t* linear_to_srgb) { tables(); memcpy(srgb_to_linear, s2l, sizeof(s2l)); memcpy(linear_to_srgb, l2s, sizeof(l2s)); }

static uint8_t clip8(coef_t v) { return v < 0 ? 0 : v > 255 ? 255 : (uint8_t)v; }
static uint8_t lin_to_srgb(int32_t v)
{
    if (v <= 0) return 0;
    if (v >= 65535) return 0xFF;
    int vmul = v * 511, off = vmul >> 16, frac = vmul & 65535, base = l2s[off];
    return (uint8_t)(base + ((frac * (l2s[off + 1] - base)) >> 16));
}
static int32_t to_i32(int64_t v) { return (int32_t)(uint32_t)(uint64_t)v; }
static int cbrt01(int v)
{
    if (v <= 0) return 0;
    if (v >= 65535) return 65535;
    int64_t root = ((v * (((v * (v - 144107LL)) >> 16) + 132114LL)) >> 16) + 14379LL;
    for (int i = 0; i < 2; ++i) {
        int64_t n = root * root * root, den = v + (n >> 31);
        root = (root * (2LL * v + (n >> 32))) / den;
    }
    return (int)root;
}

static void color_decode(const coef_t* d, size_t w, size_t h, int mode, uint8_t* out)
{
    size_t n = w * h;
    const coef_t *p0 = d, *p1 = d + n, *p2 = d + 2 * n;
    tables();
    for (size_t i = 0; i < n; ++i) {
        if (mode == 0) out[i] = clip8((coef_t)(p0[i] + 128));
        else if (mode == 1) {
            coef_t Y = (coef_t)(p0[i] + 128), Co = p1[i], Cg = p2[i];
            coef_t B = (coef_t)(Y + ((1 - Cg) >> 1) - (Co >> 1));
            coef_t G = (coef_t)(Y - ((-(int)Cg) >> 1));
            coef_t R = (coef_t)(Co + B);
            out[3 * i] = clip8(R); out[3 * i + 1] = clip8(G); out[3 * i + 2] = clip8(B);
        } else if (mode == 2) {
            coef_t L = (coef_t)(p0[i] + 2048), a = p1[i], b = p2[i];
            int64_t l_ = L * 16 + ((25974LL * a + 14143LL * b) >> 12);
            int64_t m_ = L * 16 + ((-6918LL * a - 4185LL * b) >> 12);
            int64_t s_ = L * 16 + ((-5864LL * a - 84638LL * b) >> 12);
            int64_t l = (l_ * l_ * l_) >> 32, m = (m_ * m_ * m_) >> 32, s = (s_ * s_ * s_) >> 32;
            out[3 * i]     = lin_to_srgb(to_i32((267169LL * l - 216771LL * m + 15137LL * s) >> 16));
            out[3 * i + 1] = lin_to_srgb(to_i32((-83127LL * l + 171030LL * m - 22368LL * s) >> 16));
            out[3 * i + 2] = lin_to_srgb(to_i32((-275LL * l - 46099LL * m + 111909LL * s) >> 16));
        } else {
            coef_t Y = (coef_t)(p0[i] + 221), c0 = p1[i], c1 = p2[i];
            coef_t R = (coef_t)((33779 * Y - 52830 * c0 + 19051 * c1) >> 16);
            coef_t G = (coef_t)((41184 * Y + 8188 * c0 - 50317 * c1) >> 16);
            coef_t B = (coef_t)((38182 * Y + 37906 * c0 + 37420 * c1) >> 16);
            out[3 * i] = clip8(R); out[3 * i + 1] = clip8(G); out[3 * i + 2] = clip8(B);
        }
    }
}
static void color_encode(const uint8_t* in, size_t w, size_t h, int mode, coef_t* d)
{
    size_t n = w * h;
    coef_t *p0 = d, *p1 = d + n, *p2 = d + 2 * n;
    tables();
    for (size_t i = 0; i < n; ++i) {
        if (mode == 0) { p0[i] = (coef_t)((coef_t)in[i] - 128); continue; }
        coef_t R = in[3 * i], G = in[3 * i + 1], B = in[3 * i + 2];
        if (mode == 1) {
            coef_t t = (coef_t)((R + B) >> 1);
            p0[i] = (coef_t)(((t + G) >> 1) - 128); p1[i] = (coef_t)(R - B); p2[i] = (coef_t)(G - t);
        } else if (mode == 2) {
            int r = s2l[R], g = s2l[G], b = s2l[B];
            int l = cbrt01((int)((27015LL * r + 35149LL * g + 3372LL * b) >> 16));
            int m = cbrt01((int)((13887LL * r + 44610LL * g + 7038LL * b) >> 16));
            int s = cbrt01((int)((5787LL * r + 18462LL * g + 41286LL * b) >> 16));
            p0[i] = (coef_t)(((862LL * l + 3250LL * m - 17LL * s + 32767) >> 16) - 2048);
            p1[i] = (coef_t)((8100LL * l - 9945LL * m + 1845LL * s + 32767) >> 16);
            p2[i] = (coef_t)((106LL * l + 3205LL * m - 3311LL * s + 32767) >> 16);
        } else {
            p0[i] = (coef_t)(((33779 * R + 41184 * G + 38182 * B) >> 16) - 221);
            p1[i] = (coef_t)((-52830 * R + 8188 * G + 37906 * B) >> 16);
            p2[i] = (coef_t)((19051 * R - 50317 * G + 37420 * B) >> 16);
        }
    }
}

/* ---- the 5/3 integer wavelet, as the reference walks it ---- */
static void idwt_row(coef_t* data, coef_t* scratch, size_t width)
{
    if (width < 4) return;
    coef_t *odds, *evens = scratch, *l_band = data, *h_band;
    int cf0, cf1, cf2, cf3;
    size_t half_w = width >> 1, stride = half_w, w = half_w - 1, i;
    int odd_w = (int)(width & 1);
    if (odd_w) ++stride;
    odds = scratch + stride; h_band = data + stride;
    cf1 = h_band[0];
    cf0 = l_band[0] - ((cf1 + 1) >> 1);
    evens[0] = (coef_t)cf0;
    for (i = 1; i < w; ++i) {
        cf2 = l_band[i]; cf3 = h_band[i];
        cf2 -= (cf1 + cf3 + 2) >> 2;
        evens[i] = (coef_t)cf2;
        odds[i - 1] = (coef_t)(cf1 - ((-(cf0 + cf2)) >> 1));
        ++i;
        cf0 = l_band[i]; cf1 = h_band[i];
        cf0 -= (cf1 + cf3 + 2) >> 2;
        evens[i] = (coef_t)cf0;
        odds[i - 1] = (coef_t)(cf3 - ((-(cf0 + cf2)) >> 1));
    }
    evens[w] = (coef_t)(l_band[w] - ((h_band[w - 1] + h_band[w] + 2) >> 2));
    odds[w - 1] = (coef_t)(h_band[w - 1] - ((-(evens[w - 1] + evens[w])) >> 1));
    if (odd_w) evens[w + 1] = (coef_t)(l_band[w + 1] - ((h_band[w] + 1) >> 1));
    odds[w] = (coef_t)(h_band[w] - (odd_w ? ((-(evens[w] + evens[w + 1])) >> 1) : -(int)evens[w]));
    for (i = 0; i < half_w; ++i) { data[2 * i] = evens[i]; data[2 * i + 1] = odds[i]; }
    if (odd_w) data[2 * half_w] = evens[half_w];
}
static void idwt_level(coef_t* data, coef_t* scratch, size_t width, size_t height, size_t stride)
{
    int H = (int)height - 1;
    coef_t *nn = data + mirror(-2, H) * stride, *n = data + mirror(-1, H) * stride;
    for (int i = -1; i <= (int)height; i += 2) {
        coef_t *r = data + mirror(i + 1, H) * stride, *s = data + mirror(i + 2, H) * stride;
        if (n <= s) for (size_t k = 0; k < width; ++k) r[k] = (coef_t)(r[k] - (((int)n[k] + (int)s[k] + 2) >> 2));
        if (nn <= r) for (size_t k = 0; k < width; ++k) n[k] = (coef_t)(n[k] + (((int)nn[k] + (int)r[k]) >> 1));
        if (i - 1 >= 0) idwt_row(nn, scratch, width);
        if (nn <= r) idwt_row(n, scratch, width);
        nn = r; n = s;
    }
}
static void dwt_row(coef_t* data, coef_t* scratch, size_t width)
{
    if (width < 4) return;
    coef_t *odds, *evens = scratch, *l_band = data, *h_band;
    int cf0, cf1, cf2, cf3;
    size_t half_w = width >> 1, stride = half_w, w = half_w - 1, i;
    int odd_w = (int)(width & 1);
    if (odd_w) ++stride;
    odds = scratch + stride; h_band = data + stride;
    for (i = 0; i < half_w; ++i) { evens[i] = data[2 * i]; odds[i] = data[2 * i + 1]; }
    if (odd_w) evens[half_w] = data[2 * half_w];
    cf0 = evens[0]; cf2 = evens[1];
    cf1 = (coef_t)(odds[0] + ((-(cf0 + cf2)) >> 1));
    h_band[0] = (coef_t)cf1;
    cf0 += (cf1 + 1) >> 1;
    l_band[0] = (coef_t)cf0;
    for (i = 1; i < w; ++i) {
        cf3 = odds[i]; cf0 = evens[i + 1];
        cf3 += (-(cf2 + cf0)) >> 1;
        h_band[i] = (coef_t)cf3;
        cf2 += (cf1 + cf3 + 2) >> 2;
        l_band[i] = (coef_t)cf2;
        ++i;
        cf1 = odds[i]; cf2 = evens[i + 1];
        cf1 += (-(cf2 + cf0)) >> 1;
        h_band[i] = (coef_t)cf1;
        cf0 += (cf1 + cf3 + 2) >> 2;
        l_band[i] = (coef_t)cf0;
    }
    cf3 = odds[w] + (odd_w ? ((-(evens[w] + evens[w + 1])) >> 1) : -(int)evens[w]);
    h_band[w] = (coef_t)cf3;
    l_band[w] = (coef_t)(evens[w] + ((h_band[w - 1] + cf3 + 2) >> 2));
    if (odd_w) l_band[w + 1] = (coef_t)(evens[w + 1] + ((cf3 + 1) >> 1));
}
static void dwt_level(coef_t* data, coef_t* scratch, size_t width, size_t height, size_t stride)
{
    int H = (int)height - 1;
    coef_t *nnn = data + mirror(-3, H) * stride, *nn = data + mirror(-2, H) * stride;
    for (int i = -2; i < (int)height; i += 2) {
        coef_t *n = data + mirror(i + 1, H) * stride, *r = data + mirror(i + 2, H) * stride;
        if (nn <= r) dwt_row(n, scratch, width);
        if (i + 2 < (int)height) dwt_row(r, scratch, width);
        if (nn <= r) for (size_t k = 0; k < width; ++k) n[k] = (coef_t)(n[k] - (((int)nn[k] + (int)r[k]) >> 1));
        if (nnn <= n) for (size_t k = 0; k < width; ++k) nn[k] = (coef_t)(nn[k] + (((int)nnn[k] + (int)n[k] + 2) >> 2));
        nnn = n; nn = r;
    }
}

/* the pixel stage on a copy of the coefficients: out is w * h * planes bytes.  0 = ok */
long sqzref_pixels(const int16_t* coeffs, long w, long h, int mode, int levels, uint8_t* out)
{
    size_t planes = kPlanes[mode & 3], n = (size_t)w * (size_t)h;
    coef_t* d = (coef_t*)malloc(n * planes * sizeof(coef_t));
    coef_t* scratch = (coef_t*)malloc((size_t)w * sizeof(coef_t));
    if (!d || !scratch) { free(d); free(scratch); return -1; }
    for (size_t i = 0; i < n * planes; ++i) d[i] = (coef_t)((coeffs[i] & 1) ? -(coeffs[i] >> 1) : coeffs[i] >> 1);
    for (size_t p = 0; p < planes; ++p)
        for (int level = levels - 1; level >= 0; --level) {
            size_t lw = (size_t)w, lh = (size_t)h;
            for (int l = level; l > 0; --l) { lw = (lw + 1) >> 1; lh = (lh + 1) >> 1; }
            idwt_level(d + p * n, scratch, lw, lh, (size_t)w << level);
        }
    color_decode(d, (size_t)w, (size_t)h, mode, out);
    free(d); free(scratch);
    return 0;
}

/* SQZ_encode from tight rows; dst must hold `budget` zeroed bytes.  Returns the bytes used, or -1 */
long sqzref_encode(const uint8_t* pixels, long w, long h, int mode, int levels, int scan, int subsampling, uint8_t* dst, long budget)
{
    if (w < MIN_DIM || w > MAX_DIM || h < MIN_DIM || h > MAX_DIM || mode < 0 || mode > 3 || scan < 0 || scan > 3 || levels < 1 || levels > MAX_LEVEL) return -1;
    unsigned max_level = ilog2u((unsigned)(w > h ? h : w)) - 3u;
    if (max_level > MAX_LEVEL) max_level = MAX_LEVEL;
    if ((unsigned)levels > max_level) levels = (int)max_level;
    ctx_t* c = (ctx_t*)calloc(1, sizeof(ctx_t));
    if (!c) return -1;
    c->width = (size_t)w; c->height = (size_t)h; c->mode = mode; c->scan = scan; c->levels = (size_t)levels; c->subsampling = !!subsampling; c->planes = kPlanes[mode];
    memset(dst, 0, (size_t)budget);
    bb_init(&c->buf, dst, (size_t)budget);
    bitbuf_t* b = &c->buf;
    bb_write_bits(b, MAGIC, 8); bb_write_bits(b, (unsigned)(w - 1), 16); bb_write_bits(b, (unsigned)(h - 1), 16);
    bb_write_bits(b, (unsigned)mode, 2); bb_write_bits(b, (unsigned)(levels - 1), 3); bb_write_bits(b, (unsigned)scan, 2); bb_write_bit(b, (unsigned)!!subsampling);
    long used = -1;
    coef_t* scratch = (coef_t*)malloc((size_t)w * sizeof(coef_t));
    if (!bb_eob(b) && scratch && !init_context(c)) {
        color_encode(pixels, c->width, c->height, mode, c->data);
        for (size_t p = 0; p < c->planes; ++p) {
            size_t lw = c->width, lh = c->height;
            for (size_t level = 0; level < c->levels; ++level) { dwt_level(c->plane[p], scratch, lw, lh, c->width << level); lw = (lw + 1) >> 1; lh = (lh + 1) >> 1; }
        }
        size_t n = c->width * c->height * c->planes;
        for (size_t i = 0; i < n; ++i) c->data[i] = (coef_t)(c->data[i] < 0 ? (-2 * c->data[i]) | 1 : 2 * c->data[i]);
        if (run_schedule(c, enc_bitplane) >= 0) used = (long)(((size_t)(b->ptr - b->data) * 8 + b->index + 7) / 8);
    }
    free(scratch);
    free_context(c);
    free(c);
    return used;
}

/* the LIP order of a w x h subband: xy holds w * h pairs.  Returns the count */
long sqzref_scan(int order, long w, long h, uint16_t* xy)
{
    ctx_t* c = (ctx_t*)calloc(1, sizeof(ctx_t));
    band_t* b = &c->band[0][0][0];
    c->scan = order; b->width = (size_t)w; b->height = (size_t)h;
    long k = 0;
    if (!init_subband(c, b)) for (int px = b->LIP.head; px >= 0; px = b->nodes[px].next) { xy[2 * k] = b->nodes[px].x; xy[2 * k + 1] = b->nodes[px].y; ++k; }
    free(b->nodes); free(c);
    return k;
}

int sqzref_selftest(void) { volatile int m = -3; return (m >> 1) == -2 && (int16_t)(uint16_t)0x8000u == -32768; }
