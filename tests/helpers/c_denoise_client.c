/* c_denoise_client.c — the denoiser's part of the C-ABI from a C99 caller (include/zdr.h alone, no Python in the process).
 *   c_denoise_client --check    calls zdr_denoise_workspace_bytes, zdr_denoise and zdr_denoise_backward with arguments the library
 *                               must refuse before it touches a device, and with valid parameters for the size query; prints one
 *                               line per case and "ok", exit status 0, when every answer is the expected one.
 * The pointers handed over are never dereferenced: every case is refused by the argument checks. */
#include <stdio.h>
#include <string.h>

#include "zdr.h"

static int expect(const char *what, int got, int want) {
    printf("%-28s %s (%d): %s\n", what, got == want ? "as expected" : "UNEXPECTED", got, zdr_last_error());
    return got == want ? 0 : 1;
}

int main(int argc, char **argv) {
    zdr_denoise_params p;
    float *a = (float *)(size_t)4096, *b = (float *)(size_t)8192, *c = (float *)(size_t)12288;
    void *ws = (void *)(size_t)16384;
    int bad = 0;
    size_t small, large;
    if (argc != 2 || strcmp(argv[1], "--check") != 0) {
        fprintf(stderr, "usage: %s --check\n", argv[0]);
        return 1;
    }
    memset(&p, 0, sizeof p);
    p.struct_size = (uint32_t)sizeof p; p.width = 37; p.height = 29; p.levels = 4;
    p.sigma_normal = 0.25f; p.sigma_depth = 0.1f; p.sigma_albedo = 0.0f;
    small = zdr_denoise_workspace_bytes(&p);
    p.width = 74;
    large = zdr_denoise_workspace_bytes(&p);
    p.width = 37;
    printf("workspace %lu -> %lu bytes\n", (unsigned long)small, (unsigned long)large);
    bad += !(small >= (size_t)37 * 29 * 48 && large > small);
    p.levels = 7;
    bad += expect("levels = 7", zdr_denoise(&p, a, b, c, ws, NULL), ZDR_E_INVALID);
    bad += zdr_denoise_workspace_bytes(&p) != 0;
    p.levels = 4; p.height = 0;
    bad += expect("height = 0", zdr_denoise_backward(&p, a, b, c, ws, NULL), ZDR_E_INVALID);
    p.height = 29; p.struct_size -= 4;
    bad += expect("struct_size short", zdr_denoise(&p, a, b, c, ws, NULL), ZDR_E_INVALID);
    p.struct_size += 4;
    bad += expect("null workspace", zdr_denoise(&p, a, b, c, NULL, NULL), ZDR_E_INVALID);
    bad += expect("misaligned image", zdr_denoise_backward(&p, a, b + 1, c, ws, NULL), ZDR_E_INVALID);
    bad += expect("out is the image", zdr_denoise(&p, a, b, b, ws, NULL), ZDR_E_INVALID);
    if (bad) return 2;
    printf("ok\n");
    return 0;
}
