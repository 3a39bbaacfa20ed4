/* bmp_abi_layout.c -- sizeof / offsetof of gamut_hip_bmp_info as the C compiler lays it out, in the format of abi_layout.c:
 *     <struct> <sizeof> <field>=<offset> ...
 * tests/test_bmp_cpu.py compares the numbers with the static assert and the declaration in bindings/gamut_hip.d. */
#include <stddef.h>
#include <stdio.h>
#include "gamut_hip.h"

#define F(f) printf(" %s=%zu", #f, offsetof(gamut_hip_bmp_info, f))

int main(void)
{
    printf("gamut_hip_bmp_info %zu", sizeof(gamut_hip_bmp_info));
    F(width); F(height); F(bpp); F(header_size); F(compression); F(channels_in_file); F(top_down); F(pixel_offset); F(palette_size);
    F(mask_r); F(mask_g); F(mask_b); F(mask_a); F(pixels_per_meter_x); F(pixels_per_meter_y); F(pixel_aspect_ratio);
    printf("\n");
    return 0;
}
