/* qoix_abi_layout.c -- sizeof / offsetof of gamut_hip_qoix_info as the C compiler lays it out, in the format of abi_layout.c:
 *     <struct> <sizeof> <field>=<offset> ...
 * tests/test_qoix_cpu.py compares the numbers with the static assert and the declaration in bindings/gamut_hip.d. */
#include <stddef.h>
#include <stdio.h>
#include "gamut_hip.h"

#define F(f) printf(" %s=%zu", #f, offsetof(gamut_hip_qoix_info, f))

int main(void)
{
    printf("gamut_hip_qoix_info %zu", sizeof(gamut_hip_qoix_info));
    F(width); F(height); F(version); F(channels); F(bitdepth); F(colorspace); F(compression); F(pixel_aspect_ratio); F(resolution_y);
    F(orig); F(pixel_type); F(detected);
    printf("\n");
    return 0;
}
