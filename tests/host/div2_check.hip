// Host-side check of the two-wide division of mortal_amd/csrc/mj_algo.h (no GPU needed): sp_div_domain2 gives, in either
// component, the bits of sp_div_domain -- over the SP kernel's whole operand domain (the enumeration of algo_check.hip:
// prob = tsumo_prob[c][j] * not_tsumo[s][j] / not_tsumo[s][i] for every wall size, required-tile sum, count and turn pair) and
// for the three reciprocal estimates v_rcp_f32 may return (RN(1/b) and both neighbours).
//   hipcc --offload-arch=gfx950 -O2 -std=c++17 -ffp-contract=off -o div2_check tests/host/div2_check.hip && ./div2_check
// (add -Xarch_host -fsanitize=address,undefined for the sanitized build: the program is stand-alone)
#include <hip/hip_runtime.h>
#define MJD __host__ __device__ inline
#define MJDN __device__ __noinline__
#define __popcll(x) __builtin_popcountll(x)
#define __popc(x) __builtin_popcount(x)
#include "../../mortal_amd/csrc/mj_algo.h"

#include <cmath>
#include <cstdio>
#include <cstring>

static u32 bits(float x) {
    u32 u;
    memcpy(&u, &x, 4);
    return u;
}

int main() {
    long nd = 0;
    float other = 0.f;  // the neighbour component: the previous numerator of the enumeration (0 first: the parked rows' zero fill)
    for (int n_left = 1; n_left <= 123; n_left++)
        for (int sumreq = 0; sumreq <= n_left; sumreq++) {
            const int T = n_left < 17 ? n_left : 17;
            float nt[17], tp[4][17];
            for (int j = 0; j < 17; j++) nt[j] = 0.f;
            nt[0] = 1.f;
            const int lim = (T - 1) < (n_left - sumreq) ? (T - 1) : (n_left - sumreq);
            for (int j = 0; j < lim; j++) nt[j + 1] = nt[j] * (float)(n_left - sumreq - j) / (float)(n_left - j);
            for (int c = 0; c < 4; c++)
                for (int j = 0; j < T; j++) tp[c][j] = (float)(c + 1) / (float)(n_left - j);
            for (int c = 0; c < 4; c++)
                for (int i = 0; i < T; i++)
                    for (int j = i; j < T; j++) {
                        if (nt[i] == 0.f) continue;
                        const float a = tp[c][j] * nt[j], b = nt[i], r = 1.0f / b;
                        for (int k = -1; k <= 2; k++) {  // k = 2: the kernel's own hoisted reciprocal
                            const float r0 = k < 0 ? nextafterf(r, 0.f) : k == 1 ? nextafterf(r, 2.f * r) : r;
                            const float e0 = __builtin_fmaf(-b, r0, 1.0f);
                            const float r1 = k == 2 ? sp_rcp_refined(b) : __builtin_fmaf(e0, r0, r0);
                            const float want = sp_div_domain(a, b, r1), want_o = sp_div_domain(other, b, r1);
                            const MjF2 lo = sp_div_domain2(MjF2{a, other}, b, r1), hi = sp_div_domain2(MjF2{other, a}, b, r1);
                            if (bits(lo[0]) != bits(want) || bits(hi[1]) != bits(want) || bits(lo[1]) != bits(want_o) ||
                                bits(hi[0]) != bits(want_o)) {
                                printf("sp_div_domain2 mismatch: a=%a other=%a b=%a k=%d want %a / %a got {%a, %a} {%a, %a}\n", a, other, b, k,
                                       want, want_o, lo[0], lo[1], hi[0], hi[1]);
                                return 4;
                            }
                        }
                        const MjF2 pad = sp_div_domain2(MjF2{0.f, 0.f}, b, sp_rcp_refined(b));  // a padded term adds exactly +0
                        if (bits(pad[0]) != 0u || bits(pad[1]) != 0u) return 5;
                        other = a;
                        nd++;
                    }
        }
    printf("sp_div_domain2 == sp_div_domain in both components on %ld operand pairs\n", nd);
    return 0;
}
