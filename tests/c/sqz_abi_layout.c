/* sqz_abi_layout.c -- sizeof / offsetof of gamut_hip_sqz_info and gamut_hip_sqz_desc as the C compiler lays them out, a line each in
 * the format of abi_layout.c:
 *     <struct> <sizeof> <field>=<offset> ...
 * tests/test_sqz_cpu.py compares the numbers with the static asserts in bindings/gamut_hip.d and the ctypes mirrors. */
#include <stddef.h>
#include <stdio.h>
#include "gamut_hip.h"

#define F(f) printf(" %s=%zu", #f, offsetof(gamut_hip_sqz_info, f))
#define G(f) printf(" %s=%zu", #f, offsetof(gamut_hip_sqz_desc, f))

int main(void)
{
    printf("gamut_hip_sqz_info %zu", sizeof(gamut_hip_sqz_info));
    F(width); F(height); F(planes); F(color_mode); F(levels); F(scan_order); F(subsampling); F(pixel_type); F(detected);
    printf("\ngamut_hip_sqz_desc %zu", sizeof(gamut_hip_sqz_desc));
    G(width); G(height); G(color_mode); G(levels); G(coeff_offset);
    printf("\n");
    return 0;
}
