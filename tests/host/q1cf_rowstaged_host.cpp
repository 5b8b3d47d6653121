// Stand-alone host program around the row-staged closed-form 2-D Q1 element (q1cf_stage / q1cf_elem, diffnet_amd/csrc/poisson_elem.h):
// the march of poisson2d_q1_cf.hip over one small mesh on the CPU, with the very inline functions the kernel calls.
//
//     q1cf_rowstaged_host <in> <out>
// in : int32 B, ny, nx, has_nu, has_f; float32 xm[4], ym[4], px[2], sy[2], pn0, s0, cx[3], cy[3], alpha, nb (= -beta);
//      float32 u[B][ny][nx] (Dirichlet values applied), nu[B][ny][nx] (has_nu), f[B][ny][nx] (has_f)
// out: float64 e1, e2 (sum W nu |grad u|^2, sum W f u); float32 g[B][ny][nx] (nodal contributions, Dirichlet rows not zeroed)
// (tests/test_q1cf_rowstaged.py builds it with the host side of hipcc, writes the input and compares the output with the oracle.)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "poisson_elem.h"

static bool rd(FILE* fp, void* p, size_t n) { return fread(p, 1, n, fp) == n; }

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = fopen(argv[1], "rb");
    if (!fi) return 3;
    int hd[5];
    float xm[4], ym[4], px[2], sy[2], pn0, s0, cx[3], cy[3], ab[2];
    if (!rd(fi, hd, sizeof hd) || !rd(fi, xm, sizeof xm) || !rd(fi, ym, sizeof ym) || !rd(fi, px, sizeof px) || !rd(fi, sy, sizeof sy) ||
        !rd(fi, &pn0, 4) || !rd(fi, &s0, 4) || !rd(fi, cx, sizeof cx) || !rd(fi, cy, sizeof cy) || !rd(fi, ab, sizeof ab))
        return 4;
    const int B = hd[0], ny = hd[1], nx = hd[2];
    const bool has_nu = hd[3] != 0, has_f = hd[4] != 0;
    if (B < 1 || ny < 2 || nx < 2 || B > 64 || ny > 4096 || nx > 4096) return 5;
    const size_t N = (size_t)B * ny * nx;
    std::vector<float> u(N), nu(has_nu ? N : 0), f(has_f ? N : 0), g(N, 0.f);
    if (!rd(fi, u.data(), 4 * N) || (has_nu && !rd(fi, nu.data(), 4 * N)) || (has_f && !rd(fi, f.data(), 4 * N))) return 6;
    fclose(fi);

    const int nelx = nx - 1;
    double e1 = 0.0, e2 = 0.0;
    std::vector<float> du[2], pn[2], gx[2];
    for (int k = 0; k < 2; ++k) { du[k].resize(nelx); pn[k].resize(nelx); gx[k].resize(nx); }
    auto stage = [&](int b, int y, int k) {          // what the kernel does when a node row lands
        const float* ur = &u[((size_t)b * ny + y) * nx];
        for (int e = 0; e < nelx; ++e) {
            const float* nr = has_nu ? &nu[((size_t)b * ny + y) * nx] : nullptr;
            if (nr) {
                dn::q1cf_stage(px[0], px[1], ur[e], ur[e + 1], nr[e], nr[e + 1], du[k][e], pn[k][e]);
            } else {
                du[k][e] = ur[e + 1] - ur[e];
                pn[k][e] = pn0;
            }
        }
        for (int n = 0; n < nx; ++n) gx[k][n] = 0.f;
        if (has_f) {
            const float* fr = &f[((size_t)b * ny + y) * nx];
            for (int e = 0; e < nelx; ++e) {
                gx[k][e] = fmaf(cx[1], fr[e + 1], fmaf(cx[0], fr[e], gx[k][e]));
                gx[k][e + 1] = fmaf(cx[2], fr[e + 1], cx[1] * fr[e]);
            }
        }
    };
    for (int b = 0; b < B; ++b) {
        stage(b, 0, 0);
        for (int y = 0; y + 1 < ny; ++y) {
            const int L = y & 1, U = L ^ 1;
            stage(b, y + 1, U);
            const size_t lo = ((size_t)b * ny + y) * nx, up = lo + nx;
            float le1 = 0.f, le2 = 0.f;
            if (has_f) {
                for (int n = 0; n < nx; ++n) {
                    const float tlo = fmaf(cy[1], gx[U][n], cy[0] * gx[L][n]), tup = fmaf(cy[2], gx[U][n], cy[1] * gx[L][n]);
                    g[lo + n] = fmaf(ab[1], tlo, g[lo + n]);
                    g[up + n] = fmaf(ab[1], tup, g[up + n]);
                    le2 = fmaf(u[up + n], tup, fmaf(u[lo + n], tlo, le2));
                }
            }
            for (int e = 0; e < nelx; ++e) {
                const float V0 = u[up + e] - u[lo + e], V1 = u[up + e + 1] - u[lo + e + 1];
                const float S0 = has_nu ? fmaf(sy[1], nu[up + e], sy[0] * nu[lo + e]) : s0;
                const float S1 = has_nu ? fmaf(sy[1], nu[up + e + 1], sy[0] * nu[lo + e + 1]) : s0;
                dn::q1cf_elem(xm, ym, du[L][e], du[U][e], pn[L][e], pn[U][e], V0, V1, S0, S1, ab[0], g[lo + e], g[lo + e + 1], g[up + e], g[up + e + 1], le1);
            }
            e1 += (double)le1;
            e2 += (double)le2;
        }
    }
    FILE* fo = fopen(argv[2], "wb");
    if (!fo) return 7;
    const double es[2] = {e1, e2};
    fwrite(es, sizeof es, 1, fo);
    fwrite(g.data(), 4, N, fo);
    fclose(fo);
    return 0;
}
