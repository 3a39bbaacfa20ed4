/* sqz_encode_abi_layout.c -- sizeof / offsetof of gamut_hip_sqz_encode_desc as the C compiler lays it out, in the format of abi_layout.c:
 *     <struct> <sizeof> <field>=<offset> ...
 * tests/test_sqz_encode_cpu.py compares the numbers with the static assert in bindings/gamut_hip.d and the ctypes mirror. */
#include <stddef.h>
#include <stdio.h>
#include "gamut_hip.h"

#define F(f) printf(" %s=%zu", #f, offsetof(gamut_hip_sqz_encode_desc, f))

int main(void)
{
    printf("gamut_hip_sqz_encode_desc %zu", sizeof(gamut_hip_sqz_encode_desc));
    F(width); F(height); F(color_mode); F(levels); F(scan_order); F(subsampling); F(budget);
    printf("\n");
    return 0;
}
