/* A strict C99 consumer of the JPEG encode entry points: the write callback type, the bound, a refusal that never calls the
 * callback.  Without a device the encode itself fails loudly (checked by the caller through the printed counts). */
#include <stdio.h>
#include <stdint.h>
#include "gamut_hip.h"

struct sink { long bytes; int calls; };

static void on_write(void* context, const void* data, int size)
{
    struct sink* s = (struct sink*)context;
    (void)data;
    s->bytes += size;
    s->calls += 1;
}

int main(void)
{
    static uint8_t px[16 * 16 * 3];
    struct sink s = { 0, 0 };
    gamut_hip_jpeg_write_func fn = on_write;
    int64_t bound = gamut_hip_jpeg_encode_bound(16, 16, 3, 90);
    int refused = gamut_hip_jpeg_write_to_func(fn, &s, 16, 16, 5, px, 48, 90);   /* comp 5: refused, fn never called */
    printf("bound=%lld refused=%d calls=%d\n", (long long)bound, refused, s.calls);
    return bound == 607 + 2 * ((6 * 1660 + 7) / 8) + 2 && refused == 0 && s.calls == 0 ? 0 : 1;
}
