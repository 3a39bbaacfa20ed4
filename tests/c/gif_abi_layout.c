/* gif_abi_layout.c -- sizeof / offsetof of gamut_hip_gif_info as the C compiler lays it out, in the format of abi_layout.c:
 *     <struct> <sizeof> <field>=<offset> ...
 * tests/test_gif_cpu.py compares the numbers with the static assert and the declaration in bindings/gamut_hip.d. */
#include <stddef.h>
#include <stdio.h>
#include "gamut_hip.h"

#define F(f) printf(" %s=%zu", #f, offsetof(gamut_hip_gif_info, f))

int main(void)
{
    printf("gamut_hip_gif_info %zu", sizeof(gamut_hip_gif_info));
    F(width); F(height); F(layers); F(is_gif89); F(pixel_aspect_ratio); F(fps);
    printf("\n");
    return 0;
}
