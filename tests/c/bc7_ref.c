/* bc7_ref.c -- serial restatement of saveDDS (plugins/dds.d:47-216) and of the part of bc7enc16 it runs (codecs/bc7enc16.d):
 * 64 mode-1 partitions, least squares on, the partition filterbank on, uber level 0, perceptual weights.  Written for the tests:
 * one tile at a time, every float operation a statement of its own order (build with -ffp-contract=off), every float -> int
 * conversion through f2i() with the x86-64 result.  The two selector-weight tables and the 256 x 2 table of mode 1's best endpoints
 * for one colour are computed, not typed in.
 *
 * Beyond what the issue lists as live: color_cell_compression's closing "pack the subset as its mean colour" attempt for mode 1
 * (bc7enc16.d:1304-1318) stands behind the uber-level block, not inside it, so it runs at uber level 0 and is restated here. */
#include <limits.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

typedef struct {
    int32_t mode, partition, partition_iter;          /* partition_iter: where the scan met the chosen partition, -1 when no scan ran */
    int32_t lo[2][4], hi[2][4], pbits[2][2], sel[16]; /* as handed to the bit packer (before the anchor flip) */
    u64 error;
    int32_t alpha, mode1_tried, mode1_won, single_colour, degenerate_fixed, ls_improved, early_zero, mean_colour_won;
} bc7ref_trace;

static const u32 W3[8] = { 0, 9, 18, 27, 37, 46, 55, 64 };
static const u32 W4[16] = { 0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64 };
/* bit i of entry p: the subset of pixel i in 2-subset partition p (the format's table) */
static const uint16_t PART2[64] = {
    0xCCCC, 0x8888, 0xEEEE, 0xECC8, 0xC880, 0xFEEC, 0xFEC8, 0xEC80, 0xC800, 0xFFEC, 0xFE80, 0xE800, 0xFFE8, 0xFF00, 0xFFF0, 0xF000,
    0xF710, 0x008E, 0x7100, 0x08CE, 0x008C, 0x7310, 0x3100, 0x8CCE, 0x088C, 0x3110, 0x6666, 0x366C, 0x17E8, 0x0FF0, 0x718E, 0x399C,
    0xAAAA, 0xF0F0, 0x5A5A, 0x33CC, 0x3C3C, 0x55AA, 0x9696, 0xA55A, 0x73CE, 0x13C8, 0x324C, 0x3BDC, 0x6996, 0xC33C, 0x9966, 0x0660,
    0x0272, 0x04E4, 0x4E40, 0x2720, 0xC936, 0x936C, 0x39C6, 0x639C, 0x9336, 0x9CC6, 0x817E, 0xE718, 0xCCF0, 0x0FCC, 0x7744, 0xEE22 };
static const u8 ANCHOR2[64] = {
    15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 15, 2, 8, 2, 2, 8, 8, 15, 2, 8, 2, 2, 8, 8, 2, 2,
    15, 15, 6, 8, 2, 8, 15, 15, 2, 8, 2, 2, 2, 15, 15, 6, 6, 2, 6, 8, 15, 15, 2, 2, 15, 15, 15, 15, 15, 2, 2, 15 };
/* estimate_partition's scan order (by use in a corpus; pattern 34 in slot 34) and the key partitions that admit a pattern of slots 14..34 */
static const u8 ORDER[64] = {
    0, 13, 1, 2, 15, 14, 10, 16, 3, 23, 26, 6, 7, 21, 19, 29, 8, 4, 9, 20, 5, 31, 22, 17, 18, 11, 12, 30, 24, 25, 28, 27,
    32, 33, 34, 45, 46, 51, 49, 50, 48, 38, 39, 37, 53, 52, 54, 36, 57, 58, 55, 41, 40, 42, 43, 59, 44, 56, 47, 35, 60, 63, 62, 61 };
#define B(n) (1u << (n))
static const u32 PREDICT[35] = {
    ~0u, ~0u, ~0u, ~0u, ~0u, B(1) | B(2) | B(8), B(1) | B(3) | B(7), ~0u, ~0u, B(2) | B(8) | B(16), B(7) | B(3) | B(15), ~0u,
    B(8) | B(14) | B(16), B(7) | B(14) | B(15), ~0u, ~0u, ~0u, ~0u, B(14) | B(15), B(16) | B(22) | B(14), B(17) | B(24) | B(14),
    B(2) | B(14) | B(15) | B(1), ~0u, B(1) | B(3) | B(14) | B(16) | B(22), ~0u, B(1) | B(2) | B(15) | B(17) | B(24), B(1) | B(3) | B(22),
    ~0u, ~0u, ~0u, B(14) | B(15) | B(16) | B(17), ~0u, ~0u, B(1) | B(2) | B(3) | B(27) | B(4) | B(24),
    B(14) | B(15) | B(16) | B(11) | B(17) | B(27) };
/* bc7enc16_compress_block :1837-1842 on (128, 64, 16, 32): 512, (int)(256 * 0.40322...), (int)(64 * 0.29042...), 128 */
static const u32 WEIGHT[4] = { 512, 103, 18, 128 };

static float WX3[8][4], WX4[16][4];                   /* per weight w / 64: w^2, (1 - w) w, (1 - w)^2, w -- the first three as the 6-decimal literals */
static struct { uint16_t err; u8 lo, hi; } OPT1[256][2];
static int g_ready;

static float six_decimals(double x) { return (float)(floor(x * 1e6 + 0.5) / 1e6); }

static void init_tables(void)
{
    if (g_ready) return;
    for (int k = 0; k < 24; ++k) {
        const u32 wi = k < 8 ? W3[k] : W4[k - 8];
        float* o = k < 8 ? WX3[k] : WX4[k - 8];
        const double w = wi / 64.0;
        o[0] = six_decimals(w * w); o[1] = six_decimals((1 - w) * w); o[2] = six_decimals((1 - w) * (1 - w)); o[3] = six_decimals(w);
    }
    for (int c = 0; c < 256; ++c)
        for (u32 p = 0; p < 2; ++p) {
            int best = INT_MAX;
            for (u32 lo = 0; lo < 64; ++lo)
                for (u32 hi = 0; hi < 64; ++hi) {
                    u32 low = ((lo << 1) | p) << 1, high = ((hi << 1) | p) << 1;
                    low |= low >> 7; high |= high >> 7;
                    const int v = (int)((low * (64 - W3[2]) + high * W3[2] + 32) >> 6), e = (v - c) * (v - c);
                    if (e < best) { best = e; OPT1[c][p].err = (uint16_t)e; OPT1[c][p].lo = (u8)lo; OPT1[c][p].hi = (u8)hi; }
                }
        }
    g_ready = 1;
}

/* cast(int) of a float as x86-64 does it (cvttss2si): INT_MIN for NaN and for what does not fit */
static int f2i(float f) { return f >= -2147483648.0f && f < 2147483648.0f ? (int)f : INT_MIN; }
static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
static float saturate(float v) { if (v < 0.0f) v = 0.0f; else if (v > 1.0f) v = 1.0f; return v; }      /* a NaN passes */

static u64 dist_rgb(const u8* a, const u8* b)
{
    const int l1 = a[0] * 109 + a[1] * 366 + a[2] * 37, cr1 = (a[0] << 9) - l1, cb1 = (a[2] << 9) - l1;
    const int l2 = b[0] * 109 + b[1] * 366 + b[2] * 37, cr2 = (b[0] << 9) - l2, cb2 = (b[2] << 9) - l2;
    const int dl = (l1 - l2) >> 8, dcr = (cr1 - cr2) >> 8, dcb = (cb1 - cb2) >> 8;
    return (u32)(WEIGHT[0] * (u32)(dl * dl) + WEIGHT[1] * (u32)(dcr * dcr) + WEIGHT[2] * (u32)(dcb * dcb));
}
static u64 dist_rgba(const u8* a, const u8* b)
{
    const int da = (int)a[3] - (int)b[3];
    return dist_rgb(a, b) + (u32)(WEIGHT[3] * (u32)(da * da));
}

typedef struct {                                      /* color_cell_compressor_params */
    u32 n; const u8 (*px)[4];
    u32 nw; const u32* w; const float (*wx)[4];
    u32 comp_bits; int has_alpha, share_pbit;
} cell;
typedef struct {                                      /* color_cell_compressor_results with its two selector arrays inside */
    u64 best; u8 lo[4], hi[4]; u32 pbits[2]; u8 sel[16], tmp[16];
} result;

static void scale_color(u8* out, const u8* c, const cell* p)
{
    const u32 n = p->comp_bits + 1;
    for (int i = 0; i < 4; ++i) { u32 v = (u32)c[i] << (8 - n); v |= v >> n; out[i] = (u8)v; }
}

static u64 pack_one_color(const cell* p, result* r, u32 cr, u32 cg, u32 cb, u8* sel)
{
    u32 best_err = ~0u, best_p = 0;
    for (u32 pb = 0; pb < 2; ++pb) {
        const u32 e = (u32)OPT1[cr][pb].err + OPT1[cg][pb].err + OPT1[cb][pb].err;
        if (e < best_err) { best_err = e; best_p = pb; }
    }
    const u32 c3[3] = { cr, cg, cb };
    u8 q[4];
    for (int i = 0; i < 3; ++i) {
        r->lo[i] = OPT1[c3[i]][best_p].lo; r->hi[i] = OPT1[c3[i]][best_p].hi;
        u32 low = (((u32)r->lo[i] << 1) | best_p) << 1, high = (((u32)r->hi[i] << 1) | best_p) << 1;
        low |= low >> 7; high |= high >> 7;
        q[i] = (u8)((low * (64 - W3[2]) + high * W3[2] + 32) >> 6);
    }
    r->lo[3] = r->hi[3] = 0; q[3] = 255;
    r->pbits[0] = best_p; r->pbits[1] = 0;
    memset(sel, 2, p->n);
    u64 total = 0;
    for (u32 i = 0; i < p->n; ++i) total += dist_rgb(q, p->px[i]);
    r->best = total;
    return total;
}

static u64 evaluate_solution(const u8* lo, const u8* hi, const u32* pbits, const cell* p, result* r)
{
    u8 qmin[4], qmax[4], amin[4], amax[4], wc[16][4];
    const u32 pmin = pbits[0], pmax = p->share_pbit ? pbits[0] : pbits[1];
    for (int i = 0; i < 4; ++i) { qmin[i] = (u8)((lo[i] << 1) | pmin); qmax[i] = (u8)((hi[i] << 1) | pmax); }
    scale_color(amin, qmin, p); scale_color(amax, qmax, p);
    const u32 N = p->nw, nc = p->has_alpha ? 4 : 3;
    memset(wc, 0, sizeof wc);
    memcpy(wc[0], amin, 4); memcpy(wc[N - 1], amax, 4);
    for (u32 i = 1; i < N - 1; ++i)
        for (u32 j = 0; j < nc; ++j) wc[i][j] = (u8)((amin[j] * (64 - p->w[i]) + amax[j] * p->w[i] + 32) >> 6);
    u64 total = 0;
    for (u32 i = 0; i < p->n; ++i) {
        u64 best = ~(u64)0; u32 best_sel = 0;
        for (u32 j = 0; j < N; ++j) {
            const u64 e = p->has_alpha ? dist_rgba(wc[j], p->px[i]) : dist_rgb(wc[j], p->px[i]);
            if (e < best) { best = e; best_sel = j; }
        }
        total += best;
        r->tmp[i] = (u8)best_sel;
    }
    if (total < r->best) {
        r->best = total;
        memcpy(r->lo, lo, 4); memcpy(r->hi, hi, 4);
        r->pbits[0] = pbits[0]; r->pbits[1] = pbits[1];
        memcpy(r->sel, r->tmp, p->n);
    }
    return total;
}

static int fix_degenerate(u32 mode, u8* mn, u8* mx, const float* xl, const float* xh, u32 iscale)
{
    int changed = 0;
    if (mode != 1) return 0;
    for (int i = 0; i < 3; ++i) {
        if (mn[i] != mx[i] || !(fabsf(xl[i] - xh[i]) > 0.0f)) continue;
        if (mn[i] > (iscale >> 1)) {
            if (mn[i] > 0) { mn[i]--; changed = 1; }
            else if (mx[i] < iscale) { mx[i]++; changed = 1; }
        } else {
            if (mx[i] < iscale) { mx[i]++; changed = 1; }
            else if (mn[i] > 0) { mn[i]--; changed = 1; }
        }
    }
    return changed;
}

/* one endpoint component for p-bit pb: the D text multiplies and adds in int, which wraps */
static u8 quant_pbit(float x, float scalep, int pb, int iscalep)
{
    const float a = x * scalep, b = a - (float)pb, c = b / 2.0f, d = c + .5f;
    const int v = (int)((u32)f2i(d) * 2u + (u32)pb);
    return (u8)clampi(v, pb, iscalep - 1 + pb);
}

static u64 find_optimal_solution(u32 mode, const float* xl_in, const float* xh_in, const cell* p, result* r, bc7ref_trace* t)
{
    float xl[4], xh[4];
    for (int c = 0; c < 4; ++c) { xl[c] = saturate(xl_in[c]); xh[c] = saturate(xh_in[c]); }
    const int iscalep = (1 << (p->comp_bits + 1)) - 1, comps = p->has_alpha ? 4 : 3;
    const float scalep = (float)iscalep;
    u32 best_pbits[2] = { 0, 0 };
    u8 bmin[4] = { 0, 0, 0, 0 }, bmax[4] = { 0, 0, 0, 0 };
    if (!p->share_pbit) {
        float best0 = (float)1e+9, best1 = (float)1e+9;
        for (int pb = 0; pb < 2; ++pb) {
            u8 xmin[4], xmax[4], slo[4], shi[4];
            for (int c = 0; c < 4; ++c) { xmin[c] = quant_pbit(xl[c], scalep, pb, iscalep); xmax[c] = quant_pbit(xh[c], scalep, pb, iscalep); }
            scale_color(slo, xmin, p); scale_color(shi, xmax, p);
            float e0 = 0, e1 = 0;
            for (int i = 0; i < comps; ++i) {
                const float a = xl[i] * 255.0f, da = (float)slo[i] - a, b = xh[i] * 255.0f, db = (float)shi[i] - b;
                e0 += da * da; e1 += db * db;
            }
            if (e0 < best0) { best0 = e0; best_pbits[0] = (u32)pb; for (int c = 0; c < 4; ++c) bmin[c] = xmin[c] >> 1; }
            if (e1 < best1) { best1 = e1; best_pbits[1] = (u32)pb; for (int c = 0; c < 4; ++c) bmax[c] = xmax[c] >> 1; }
        }
    } else {
        float best = (float)1e+9;
        for (int pb = 0; pb < 2; ++pb) {
            u8 xmin[4], xmax[4], slo[4], shi[4];
            for (int c = 0; c < 4; ++c) { xmin[c] = quant_pbit(xl[c], scalep, pb, iscalep); xmax[c] = quant_pbit(xh[c], scalep, pb, iscalep); }
            scale_color(slo, xmin, p); scale_color(shi, xmax, p);
            float e = 0;
            for (int i = 0; i < comps; ++i) {
                const float a = (float)slo[i] / 255.0f, da = a - xl[i], b = (float)shi[i] / 255.0f, db = b - xh[i];
                const float s = da * da + db * db;
                e += s;
            }
            if (e < best) {
                best = e; best_pbits[0] = best_pbits[1] = (u32)pb;
                for (int c = 0; c < 4; ++c) { bmin[c] = xmin[c] >> 1; bmax[c] = xmax[c] >> 1; }
            }
        }
    }
    if (fix_degenerate(mode, bmin, bmax, xl, xh, (u32)iscalep >> 1)) t->degenerate_fixed = 1;
    if (r->best == ~(u64)0 || memcmp(bmin, r->lo, 4) || memcmp(bmax, r->hi, 4) || best_pbits[0] != r->pbits[0] || best_pbits[1] != r->pbits[1])
        evaluate_solution(bmin, bmax, best_pbits, p, r);
    return r->best;
}

static void normalize4(float* v)
{
    float s = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    if (s != 0.0f) { s = 1.0f / sqrtf(s); v[0] *= s; v[1] *= s; v[2] *= s; v[3] *= s; }
}
static float dot4(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }

static void least_squares(const cell* p, const u8* sel, float* xl, float* xh)
{
    const int nc = p->has_alpha ? 4 : 3;
    float z00 = 0, z10 = 0, z11 = 0, q00[4] = { 0, 0, 0, 0 }, t[4] = { 0, 0, 0, 0 };
    for (u32 i = 0; i < p->n; ++i) {
        const float* wx = p->wx[sel[i]];
        z00 += wx[0]; z10 += wx[1]; z11 += wx[2];
        const float w = wx[3];
        for (int c = 0; c < nc; ++c) { q00[c] += w * (float)p->px[i][c]; t[c] += (float)p->px[i][c]; }
    }
    const float z01 = z10;
    float det = z00 * z11 - z01 * z10;
    if (det != 0.0f) det = 1.0f / det;
    const float iz00 = z11 * det, iz01 = -z01 * det, iz10 = -z10 * det, iz11 = z00 * det;
    for (int c = 0; c < nc; ++c) {
        const float q10 = t[c] - q00[c];
        xl[c] = iz00 * q00[c] + iz01 * q10; xh[c] = iz10 * q00[c] + iz11 * q10;
    }
    if (!p->has_alpha) xl[3] = xh[3] = 255.0f;
}

static u64 color_cell_compression(u32 mode, const cell* p, result* r, bc7ref_trace* t)
{
    r->best = ~(u64)0;
    if (mode == 1) {
        int same = 1;
        for (u32 i = 1; i < p->n; ++i) if (p->px[i][0] != p->px[0][0] || p->px[i][1] != p->px[0][1] || p->px[i][2] != p->px[0][2]) { same = 0; break; }
        if (same) { t->single_colour = 1; return pack_one_color(p, r, p->px[0][0], p->px[0][1], p->px[0][2], r->sel); }
    }
    float mean[4] = { 0, 0, 0, 0 }, mean_scaled[4], axis[4];
    for (u32 i = 0; i < p->n; ++i) for (int c = 0; c < 4; ++c) mean[c] = mean[c] + (float)p->px[i][c];
    const float inv_n = 1.0f / (float)p->n, inv_n255 = 1.0f / ((float)p->n * 255.0f);
    for (int c = 0; c < 4; ++c) { mean_scaled[c] = mean[c] * inv_n; mean[c] = saturate(mean[c] * inv_n255); }
    if (p->has_alpha) {                               /* incremental PCA */
        axis[0] = axis[1] = axis[2] = axis[3] = 0.0f;
        for (u32 i = 0; i < p->n; ++i) {
            float col[4], n[4], a[4], b[4], c[4], d[4];
            for (int k = 0; k < 4; ++k) col[k] = (float)p->px[i][k] - mean_scaled[k];
            for (int k = 0; k < 4; ++k) { a[k] = col[k] * col[0]; b[k] = col[k] * col[1]; c[k] = col[k] * col[2]; d[k] = col[k] * col[3]; }
            memcpy(n, i ? axis : col, sizeof n);
            normalize4(n);
            axis[0] += dot4(a, n); axis[1] += dot4(b, n); axis[2] += dot4(c, n); axis[3] += dot4(d, n);
        }
        normalize4(axis);
    } else {                                          /* covariance and three power iterations */
        float cov[6] = { 0, 0, 0, 0, 0, 0 };
        for (u32 i = 0; i < p->n; ++i) {
            const float rr = (float)p->px[i][0] - mean_scaled[0], g = (float)p->px[i][1] - mean_scaled[1], b = (float)p->px[i][2] - mean_scaled[2];
            cov[0] += rr * rr; cov[1] += rr * g; cov[2] += rr * b; cov[3] += g * g; cov[4] += g * b; cov[5] += b * b;
        }
        float vfr = .9f, vfg = 1.0f, vfb = .7f;
        for (int iter = 0; iter < 3; ++iter) {
            float rr = vfr * cov[0] + vfg * cov[1] + vfb * cov[2];
            float g = vfr * cov[1] + vfg * cov[3] + vfb * cov[4];
            float b = vfr * cov[2] + vfg * cov[4] + vfb * cov[5];
            const float ar = fabsf(rr), ag = fabsf(g), ab = fabsf(b), m0 = ar > ag ? ar : ag;
            float m = m0 > ab ? m0 : ab;
            if (m > 1e-10f) { m = 1.0f / m; rr *= m; g *= m; b *= m; }
            vfr = rr; vfg = g; vfb = b;
        }
        float len = vfr * vfr + vfg * vfg + vfb * vfb;
        if (len < 1e-10f) axis[0] = axis[1] = axis[2] = axis[3] = 0.0f;
        else { len = 1.0f / sqrtf(len); vfr *= len; vfg *= len; vfb *= len; axis[0] = vfr; axis[1] = vfg; axis[2] = vfb; axis[3] = 0.0f; }
    }
    if (dot4(axis, axis) < .5f) {
        axis[0] = .213f; axis[1] = .715f; axis[2] = .072f; axis[3] = p->has_alpha ? .715f : 0.0f;
        normalize4(axis);
    }
    float l = 1e+9f, h = -1e+9f;
    for (u32 i = 0; i < p->n; ++i) {
        float q[4];
        for (int k = 0; k < 4; ++k) q[k] = (float)p->px[i][k] - mean_scaled[k];
        const float d = dot4(q, axis);
        l = l < d ? l : d; h = h > d ? h : d;
    }
    l *= 1.0f / 255.0f; h *= 1.0f / 255.0f;
    float mn[4], mx[4];
    for (int k = 0; k < 4; ++k) { const float b0 = axis[k] * l, b1 = axis[k] * h; mn[k] = saturate(mean[k] + b0); mx[k] = saturate(mean[k] + b1); }
    if (mn[0] + mn[1] + mn[2] + mn[3] > mx[0] + mx[1] + mx[2] + mx[3]) { float s[4]; memcpy(s, mn, 16); memcpy(mn, mx, 16); memcpy(mx, s, 16); }
    if (!find_optimal_solution(mode, mn, mx, p, r, t)) { t->early_zero = 1; return 0; }
    {
        float xl[4] = { 0, 0, 0, 0 }, xh[4] = { 0, 0, 0, 0 };
        const u64 before = r->best;
        least_squares(p, r->sel, xl, xh);
        for (int k = 0; k < 4; ++k) { xl[k] = xl[k] * (1.0f / 255.0f); xh[k] = xh[k] * (1.0f / 255.0f); }
        const u64 after = find_optimal_solution(mode, xl, xh, p, r, t);
        if (after < before) t->ls_improved = 1;
        if (!after) { t->early_zero = 1; return 0; }
    }
    if (mode == 1) {                                  /* :1304-1318 */
        result avg = *r;
        const u32 cr = (u32)f2i(.5f + mean[0] * 255.0f), cg = (u32)f2i(.5f + mean[1] * 255.0f), cb = (u32)f2i(.5f + mean[2] * 255.0f);
        const u64 e = pack_one_color(p, &avg, cr, cg, cb, r->tmp);        /* mean is finite and in [0, 1]: 0..255 */
        if (e < r->best) {
            memcpy(avg.sel, r->tmp, p->n); memcpy(avg.tmp, r->tmp, sizeof avg.tmp);
            *r = avg; r->best = e;
            t->mean_colour_won = 1;
        }
    }
    return r->best;
}

static u64 estimate_cell(u32 n, const u8 (*px)[4], u64 best_so_far)
{
    u32 lo[3] = { 255, 255, 255 }, hi[3] = { 0, 0, 0 };
    for (u32 i = 0; i < n; ++i) for (int c = 0; c < 3; ++c) { if (px[i][c] < lo[c]) lo[c] = px[i][c]; if (px[i][c] > hi[c]) hi[c] = px[i][c]; }
    int wc[8][3], dots[8], thresh[7], l1[8], cr1[8], cb1[8];
    const int a[3] = { (int)hi[0] - (int)lo[0], (int)hi[1] - (int)lo[1], (int)hi[2] - (int)lo[2] };
    for (int i = 0; i < 8; ++i) {
        for (int c = 0; c < 3; ++c) wc[i][c] = i == 0 ? (int)lo[c] : i == 7 ? (int)hi[c] : (int)(u8)((lo[c] * (64 - W3[i]) + hi[c] * W3[i] + 32) >> 6);
        dots[i] = wc[i][0] * a[0] + wc[i][1] * a[1] + wc[i][2] * a[2];
        l1[i] = wc[i][0] * 109 + wc[i][1] * 366 + wc[i][2] * 37; cr1[i] = (wc[i][0] << 9) - l1[i]; cb1[i] = (wc[i][2] << 9) - l1[i];
    }
    for (int i = 0; i < 7; ++i) thresh[i] = (dots[i] + dots[i + 1] + 1) >> 1;
    u64 total = 0;
    for (u32 i = 0; i < n; ++i) {
        const int d = a[0] * px[i][0] + a[1] * px[i][1] + a[2] * px[i][2];
        int s = 0;
        for (int k = 6; k >= 0; --k) if (d >= thresh[k]) { s = k + 1; break; }
        const int l2 = px[i][0] * 109 + px[i][1] * 366 + px[i][2] * 37, cr2 = (px[i][0] << 9) - l2, cb2 = (px[i][2] << 9) - l2;
        const int dl = (l1[s] - l2) >> 8, dcr = (cr1[s] - cr2) >> 8, dcb = (cb1[s] - cb2) >> 8;
        const int ie = (int)(WEIGHT[0] * (u32)(dl * dl) + WEIGHT[1] * (u32)(dcr * dcr) + WEIGHT[2] * (u32)(dcb * dcb));
        total += (u64)(int64_t)ie;
        if (total > best_so_far) break;
    }
    return total;
}

static u32 estimate_partition(const u8 (*px)[4], int* iter_of_best)
{
    u64 best_err = ~(u64)0;
    u32 best = 0;
    int key = 0;
    *iter_of_best = 0;
    for (u32 it = 0; it < 64 && best_err > 0; ++it) {
        const u32 part = ORDER[it];
        if (it >= 14 && it <= 34 && !(PREDICT[part] & (1u << (key + 1)))) {
            if (it == 34) break;
            continue;
        }
        u8 sub[2][16][4]; u32 n[2] = { 0, 0 };
        for (int i = 0; i < 16; ++i) { const u32 k = (PART2[part] >> i) & 1u; memcpy(sub[k][n[k]++], px[i], 4); }
        u64 total = 0;
        for (u32 k = 0; k < 2 && total < best_err; ++k) total += estimate_cell(n[k], (const u8 (*)[4])sub[k], best_err);
        if (total < best_err) { best_err = total; best = part; *iter_of_best = (int)it; }
        if (part == 34 && best != 34) break;
        if (it == 13) key = (int)best;
    }
    return best;
}

static void put_bits(u8* b, u32 val, u32 n, u32* ofs)
{
    for (u32 i = 0; i < n; ++i, ++*ofs) if ((val >> i) & 1u) b[*ofs >> 3] |= (u8)(1u << (*ofs & 7));
}

/* encode_bc7_block for modes 1 and 6 */
static void pack_block(u8* out, const bc7ref_trace* t)
{
    const u32 mode = (u32)t->mode, subsets = mode == 1 ? 2 : 1, bits = mode == 1 ? 3 : 4, num = 1u << bits;
    const u32 pmask = mode == 1 ? PART2[t->partition] : 0;
    u32 sel[16], lo[2][4], hi[2][4], pb[2][2];
    int anchor[2] = { -1, -1 };
    for (int i = 0; i < 16; ++i) sel[i] = (u32)t->sel[i];
    for (int k = 0; k < 2; ++k) for (int c = 0; c < 4; ++c) { lo[k][c] = (u32)t->lo[k][c]; hi[k][c] = (u32)t->hi[k][c]; }
    for (int k = 0; k < 2; ++k) for (int c = 0; c < 2; ++c) pb[k][c] = (u32)t->pbits[k][c];
    for (u32 k = 0; k < subsets; ++k) {
        const u32 ai = k ? ANCHOR2[t->partition] : 0;
        anchor[k] = (int)ai;
        if (sel[ai] & (num >> 1)) {
            for (int i = 0; i < 16; ++i) if (((pmask >> i) & 1u) == k) sel[i] = (num - 1) - sel[i];
            for (int c = 0; c < 4; ++c) { const u32 s = lo[k][c]; lo[k][c] = hi[k][c]; hi[k][c] = s; }
            if (mode != 1) { const u32 s = pb[k][0]; pb[k][0] = pb[k][1]; pb[k][1] = s; }
        }
    }
    memset(out, 0, 16);
    u32 ofs = 0;
    put_bits(out, 1u << mode, mode + 1, &ofs);
    if (mode == 1) put_bits(out, (u32)t->partition, 6, &ofs);
    for (u32 c = 0; c < (mode == 6 ? 4u : 3u); ++c)
        for (u32 k = 0; k < subsets; ++k) { put_bits(out, lo[k][c], mode == 6 ? 7 : 6, &ofs); put_bits(out, hi[k][c], mode == 6 ? 7 : 6, &ofs); }
    for (u32 k = 0; k < subsets; ++k) { put_bits(out, pb[k][0], 1, &ofs); if (mode != 1) put_bits(out, pb[k][1], 1, &ofs); }
    for (int i = 0; i < 16; ++i) put_bits(out, sel[i], i == anchor[0] || i == anchor[1] ? bits - 1 : bits, &ofs);
}

/* bc7enc16_compress_block on 16 rgba pixels; trace may be NULL */
void bc7ref_block(const u8* tile, u8* out16, bc7ref_trace* trace)
{
    init_tables();
    bc7ref_trace local, *t = trace ? trace : &local;
    const u8 (*px)[4] = (const u8 (*)[4])tile;
    memset(t, 0, sizeof *t);
    t->partition_iter = -1;
    for (int i = 0; i < 16; ++i) if (px[i][3] < 255) t->alpha = 1;
    cell p; result r6;
    memset(&r6, 0, sizeof r6);
    p.n = 16; p.px = px; p.nw = 16; p.w = W4; p.wx = (const float (*)[4])WX4; p.comp_bits = 7; p.has_alpha = t->alpha; p.share_pbit = 0;
    u64 best = color_cell_compression(6, &p, &r6, t);
    t->mode = 6;
    for (int c = 0; c < 4; ++c) { t->lo[0][c] = r6.lo[c]; t->hi[0][c] = r6.hi[c]; }
    t->pbits[0][0] = (int32_t)r6.pbits[0]; t->pbits[0][1] = (int32_t)r6.pbits[1];
    for (int i = 0; i < 16; ++i) t->sel[i] = r6.sel[i];
    if (!t->alpha && best > 0) {
        t->mode1_tried = 1;
        int it = 0;
        const u32 part = estimate_partition(px, &it);
        u8 sub[2][16][4], index[2][16]; u32 n[2] = { 0, 0 };
        result r1[2];
        memset(r1, 0, sizeof r1);
        for (int i = 0; i < 16; ++i) { const u32 k = (PART2[part] >> i) & 1u; memcpy(sub[k][n[k]], px[i], 4); index[k][n[k]++] = (u8)i; }
        p.nw = 8; p.w = W3; p.wx = (const float (*)[4])WX3; p.comp_bits = 6; p.share_pbit = 1;
        u64 trial = 0;
        for (u32 k = 0; k < 2; ++k) {
            p.n = n[k]; p.px = (const u8 (*)[4])sub[k];
            trial += color_cell_compression(1, &p, &r1[k], t);
            if (trial > best) break;
        }
        if (trial < best) {
            best = trial;
            t->mode1_won = 1; t->mode = 1; t->partition = (int32_t)part; t->partition_iter = it;
            for (u32 k = 0; k < 2; ++k) {
                for (u32 i = 0; i < n[k]; ++i) t->sel[index[k][i]] = r1[k].sel[i];
                for (int c = 0; c < 4; ++c) { t->lo[k][c] = r1[k].lo[c]; t->hi[k][c] = r1[k].hi[c]; }
                t->pbits[k][0] = (int32_t)r1[k].pbits[0];
            }
        }
    }
    t->error = best;
    pack_block(out16, t);
}

int64_t bc7ref_dds_size(int w, int h) { return 148 + 16 * (int64_t)((w + 3) / 4) * ((h + 3) / 4); }

static void put32(u8* p, u32 v) { p[0] = (u8)v; p[1] = (u8)(v >> 8); p[2] = (u8)(v >> 16); p[3] = (u8)(v >> 24); }

/* saveDDS: the whole file into out (bc7ref_dds_size bytes); pitch in bytes, may be negative */
void bc7ref_write_dds(const u8* pixels, int64_t pitch, int w, int h, int comp, u8* out)
{
    const int bw = (w + 3) / 4, bh = (h + 3) / 4;
    memset(out, 0, 148);
    memcpy(out, "DDS ", 4);
    put32(out + 4, 124); put32(out + 8, 0x81007); put32(out + 12, (u32)h); put32(out + 16, (u32)w);
    put32(out + 20, ((((u32)w + 3) & ~3u) * (((u32)h + 3) & ~3u) * 8u) >> 3);      /* :96, in uint: the product by 8 wraps above 2^29 pixels */
    put32(out + 76, 32); put32(out + 80, 4); put32(out + 84, 0x30315844);
    put32(out + 108, 0x1000);
    put32(out + 128, 98); put32(out + 132, 3); put32(out + 140, 1);
    for (int by = 0; by < bh; ++by)
        for (int bx = 0; bx < bw; ++bx) {
            u8 tile[16][4];
            memset(tile, 0, sizeof tile);
            for (int ly = 0; ly < 4 && by * 4 + ly < h; ++ly)
                for (int lx = 0; lx < 4 && bx * 4 + lx < w; ++lx) {
                    const u8* s = pixels + (int64_t)(by * 4 + ly) * pitch + (int64_t)(bx * 4 + lx) * comp;
                    u8* d = tile[ly * 4 + lx];
                    if (comp <= 2) { d[0] = d[1] = d[2] = s[0]; d[3] = comp == 2 ? s[1] : 255; }
                    else { d[0] = s[0]; d[1] = s[1]; d[2] = s[2]; d[3] = comp == 4 ? s[3] : 255; }
                }
            bc7ref_block(&tile[0][0], out + 148 + 16 * ((int64_t)by * bw + bx), 0);
        }
}

void bc7ref_blocks(const u8* tiles, int64_t n, u8* out, bc7ref_trace* traces)
{
    for (int64_t i = 0; i < n; ++i) bc7ref_block(tiles + 64 * i, out + 16 * i, traces ? traces + i : 0);
}

/* the computed tables: 256 x 2 x (err, lo, hi) as int32, then WX3 (8 x 4) and WX4 (16 x 4) */
void bc7ref_table(int32_t* out) { init_tables(); for (int c = 0; c < 256; ++c) for (int p = 0; p < 2; ++p) { int32_t* o = out + (c * 2 + p) * 3; o[0] = OPT1[c][p].err; o[1] = OPT1[c][p].lo; o[2] = OPT1[c][p].hi; } }
void bc7ref_weight_tables(float* wx3, float* wx4) { init_tables(); memcpy(wx3, WX3, sizeof WX3); memcpy(wx4, WX4, sizeof WX4); }
