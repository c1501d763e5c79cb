/* Stand-alone driver of tools/flow_warp_sanitize.py: reads the flow_warp cases of tests/edge_values.py from a file and runs
 * pm_flow_warp (oracle/c/pm_ops.c, the line-for-line twin of flow_warp_kernel) on each, so that the address and
 * undefined-behaviour sanitizers see every index and every float -> int cast the kernel would make.  Built by the script:
 *   gcc -O1 -g -ffp-contract=off -fno-fast-math -march=x86-64-v3 -pthread \
 *       -fsanitize=address,undefined,float-cast-overflow -fno-sanitize-recover=all \
 *       tools/flow_warp_sanitize.c oracle/c/pm_ops.c -lm -o <dir>/flow_warp_sanitize
 * Case record: int32 N, C, H, W, flowN; float32 im[N*C*H*W], flow[flowN*2*H*W], lin_x[W], lin_y[H]. */
#include <stdio.h>
#include <stdlib.h>
void pm_flow_warp(const float *im, const float *flow, const float *lin_x, const float *lin_y, float *out, int N, int C,
                  int H, int W, int flowN);
int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "rb") : NULL;
    if (!f) return 2;
    int hdr[5], cases = 0;
    unsigned long sum = 0;
    while (fread(hdr, sizeof(int), 5, f) == 5) {
        const int N = hdr[0], C = hdr[1], H = hdr[2], W = hdr[3], fn = hdr[4];
        const size_t ni = (size_t)N * C * H * W, nf = (size_t)fn * 2 * H * W;
        float *im = malloc(ni * 4), *fl = malloc(nf * 4), *lx = malloc(W * 4), *ly = malloc(H * 4), *out = malloc(ni * 4);
        if (!im || !fl || !lx || !ly || !out || fread(im, 4, ni, f) != ni || fread(fl, 4, nf, f) != nf ||
            fread(lx, 4, W, f) != (size_t)W || fread(ly, 4, H, f) != (size_t)H)
            return 3;
        pm_flow_warp(im, fl, lx, ly, out, N, C, H, W, fn);
        for (size_t i = 0; i < ni; ++i) sum += ((unsigned *)out)[i] & 0xff;          /* every output is read */
        free(im); free(fl); free(lx); free(ly); free(out);
        ++cases;
    }
    fclose(f);
    printf("%d cases, checksum %lu\n", cases, sum);
    return 0;
}
