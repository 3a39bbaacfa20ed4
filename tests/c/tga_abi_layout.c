/* tga_abi_layout.c -- sizeof / offsetof of gamut_hip_tga_info as the C compiler lays it out, in the format of abi_layout.c:
 *     <struct> <sizeof> <field>=<offset> ...
 * tests/test_tga_cpu.py compares the numbers with the static assert and the declaration in bindings/gamut_hip.d. */
#include <stddef.h>
#include <stdio.h>
#include "gamut_hip.h"

#define F(f) printf(" %s=%zu", #f, offsetof(gamut_hip_tga_info, f))

int main(void)
{
    printf("gamut_hip_tga_info %zu", sizeof(gamut_hip_tga_info));
    F(width); F(height); F(bpp); F(image_type); F(rle); F(indexed); F(rgb16); F(channels_in_file); F(bottom_up);
    F(palette_start); F(palette_len); F(cmap_size); F(data_offset); F(detected);
    printf("\n");
    return 0;
}
