// Stand-alone host check of csrc/div_const_proof.h (no HIP, no GPU), meant for a sanitizer build:
//   c++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -o div_const_proof_check tools/div_const_proof_check.cpp && ./div_const_proof_check
// The fixed list of tests/test_div_const_proof.py, 3 000 random divisors in [0.05, 1] (verdict counts printed), and
// for every proven one of the first 200 a million random dividends tried against a / sd.  Exit status 0: all as expected.
#include "../tombo_amd/csrc/div_const_proof.h"
#include <stdio.h>
#include <stdlib.h>

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t rng()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return rng_state;
}
static double from_bits(uint64_t b) { double x; memcpy(&x, &b, 8); return x; }

int main()
{
    using namespace div_const_proof;
    int bad = 0;
    const double yes[] = {0x1.69574c5f06820p-2, 0x1.cd5185c918344p-3, 0.25, 0.375, 1.0, 0x1p-200, 3.0};
    const double no[] = {0x1.e3cf63ef4d557p-1, 0.0, -0.0, -0.5, INFINITY, -INFINITY, NAN, 0x1p-1060, 0x1p-1022 / 2,
                         0x1.fffffffffffffp-1, 0x1.fffffffffffffp3, 0x1p-300, 0x1p300};
    for (double s : yes) if (proven(s) != 1) { printf("expected proven: %a\n", s); bad++; }
    for (double s : no) if (proven(s) != 0) { printf("expected unproven: %a\n", s); bad++; }
    {   // the failing pair: the two-operation form is one ulp below the quotient
        const double s = 0x1.e3cf63ef4d557p-1, a = 0x1.bca5d32101e7bp+52;
        const double yh = 1.0 / s, yl = recip_low_host(s, yh), q2 = div_const2_host(a, yh, yl), q = a / s;
        printf("failing pair: two-operation %a, quotient %a\n", q2, q);
        if (!(q2 < q && nextafter(q2, INFINITY) == q)) { printf("expected a one-ulp miss\n"); bad++; }
    }
    int n_proven = 0;
    const int n_sd = 3000;
    for (int i = 0; i < n_sd; i++) {
        const double s = 0.05 + 0.95 * (double)(rng() >> 11) * 0x1p-53;
        const int p = proven(s);
        n_proven += p;
        if (p && i < 200) {
            const double yh = 1.0 / s, yl = recip_low_host(s, yh);
            for (int k = 0; k < 1000000; k++) {
                const double a = from_bits((rng() & 0x800fffffffffffffull) | ((uint64_t)(1023 - 40 + rng() % 80) << 52));
                if (div_const2_host(a, yh, yl) != a / s) { printf("PROVEN sd %a misses at a = %a\n", s, a); bad++; break; }
            }
        }
    }
    printf("%d of %d random divisors proven\n", n_proven, n_sd);
    if (n_proven < n_sd * 9 / 10) { printf("fewer proven than expected\n"); bad++; }
    printf(bad ? "FAILED: %d\n" : "ok\n", bad);
    return bad ? 1 : 0;
}
