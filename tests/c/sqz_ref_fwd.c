/* sqz_ref_fwd.c -- the forward steps of tests/c/sqz_ref.c's encoder, exported on their own: nothing here but the include and two
 * entries that call its static color_encode, dwt_level and the sign-magnitude line of sqzref_encode.
 *   sqzref_analyze: tight l8 / rgb8 pixels -> planes * w * h sign-magnitude coefficients (what SQZ_encode holds before SQZ_schedule_task)
 *   sqzref_forward: two's-complement int16 planes in raster order -> the same, without the colour stage
 * `levels` is taken as given (the caller clamps).  0 = ok, -1 = no memory. */
#include "sqz_ref.c"

static void forward_planes(coef_t* d, size_t w, size_t h, size_t planes, int levels, coef_t* scratch)
{
    size_t n = w * h;
    for (size_t p = 0; p < planes; ++p) {
        size_t lw = w, lh = h;
        for (int level = 0; level < levels; ++level) { dwt_level(d + p * n, scratch, lw, lh, w << level); lw = (lw + 1) >> 1; lh = (lh + 1) >> 1; }
    }
    for (size_t i = 0; i < n * planes; ++i) d[i] = (coef_t)(d[i] < 0 ? (-2 * d[i]) | 1 : 2 * d[i]);
}

long sqzref_analyze(const uint8_t* pixels, long w, long h, int mode, int levels, int16_t* out)
{
    coef_t* scratch = (coef_t*)malloc((size_t)w * sizeof(coef_t));
    if (!scratch) return -1;
    color_encode(pixels, (size_t)w, (size_t)h, mode, out);
    forward_planes(out, (size_t)w, (size_t)h, kPlanes[mode & 3], levels, scratch);
    free(scratch);
    return 0;
}

long sqzref_forward(const int16_t* planes_in, long w, long h, int planes, int levels, int16_t* out)
{
    coef_t* scratch = (coef_t*)malloc((size_t)w * sizeof(coef_t));
    if (!scratch) return -1;
    memcpy(out, planes_in, (size_t)w * (size_t)h * (size_t)planes * sizeof(coef_t));
    forward_planes(out, (size_t)w, (size_t)h, (size_t)planes, levels, scratch);
    free(scratch);
    return 0;
}
