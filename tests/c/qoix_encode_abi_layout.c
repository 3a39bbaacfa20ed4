/* qoix_encode_abi_layout.c -- sizeof / offsetof of gamut_hip_qoix_desc as the C compiler lays it out, in the format of abi_layout.c:
 *     <struct> <sizeof> <field>=<offset> ...
 * tests/test_qoix_encode_cpu.py compares the numbers with the static assert and the declaration in bindings/gamut_hip.d. */
#include <stddef.h>
#include <stdio.h>
#include "gamut_hip.h"

#define F(f) printf(" %s=%zu", #f, offsetof(gamut_hip_qoix_desc, f))

int main(void)
{
    printf("gamut_hip_qoix_desc %zu", sizeof(gamut_hip_qoix_desc));
    F(width); F(height); F(channels); F(colorspace); F(mode); F(pixel_aspect_ratio); F(resolution_y);
    printf("\n");
    return 0;
}
