// div_const_proof.h -- host only, no HIP: for ONE divisor sd, is the two-operation quotient
//     q2(a) = fma(a, yh, a * yl),   yh = RN(1 / sd),   yl = RN(RN(1 - sd yh) yh)
// (div_const2 / recip_low, tba_common.h) the IEEE quotient RN(a / sd) for EVERY dividend a?
// A divisor that is a constant of the model can be asked once (tba_set_model), and where the answer is
// yes the forward pass divides in two float64 operations instead of div_by_recip's five.
//
// The error of q2 before its final rounding.  e = 1 - sd yh is exact in an fma and |e| <= 2^-53 (yh is a
// correctly rounded reciprocal).  1 / sd = yh / (1 - e) = yh (1 + e + e^2 + ...) and yl = e yh (1 + d1),
// |d1| <= 2^-53, so 1 / sd - (yh + yl) = yh (e^2 + e^3 + ... - e d1): at most 2^-106 + 2^-106 (1 + 2^-52)
// relative to yh.  p = RN(a yl) = a yl (1 + d2) adds |e| (1 + 2^-53) 2^-53 <= 2^-106 (1 + 2^-53), and
// yh = (1 / sd)(1 - e) turns "relative to yh" into "relative to 1 / sd" at a factor 1 + 2^-53.  The fma adds
// a yh + p without an error of its own.  Together the value that is rounded is (a / sd)(1 + eta) with
//     |eta| <= 3 2^-106 (1 + 2^-50).
// RN is monotone and constant between two neighbouring rounding boundaries (the midpoints of adjacent
// doubles), so RN of that value differs from RN(a / sd) only if a boundary m lies between the two:
// |m - a / sd| <= |eta| (a / sd).
//
// The dividends that come that close can be listed.  S, A: the 53-bit integer significands of sd and a
// (2^52 <= S, A < 2^53).  The quotient of the significands is A / S, in [1, 2) for A >= S and in (1/2, 1)
// below; its boundaries are M / 2^k with M odd, k = 53 for A >= S and k = 54 for A < S.  With the integer
//     rho = 2^k A - M S
// the relative distance to that boundary is |rho| / (2^k A) > |rho| 2^-106 (k = 53) or |rho| 2^-107
// (k = 54): a wrong rounding needs |rho| < 6 (1 + 2^-50), i.e. |rho| <= 6 (and rho = 0 has no solution: it
// would need 2^k | S).  The prover takes R = 64, ten times the bound, and for each k and each rho in
// [-R, R] solves 2^k A = rho (mod S) -- S = 2^t S' with S' odd: rho must be a multiple of 2^t (M odd: an
// odd one), and A = (rho / 2^t) 2^-(k - t) (mod S') -- walks the solutions on the right side of S, keeps
// those whose M is odd and tries q2 against a / sd on each, in host arithmetic (fma and division are
// correctly rounded there as on the device; the TU is built with -ffp-contract=off).  At most 2^t
// solutions per rho and 2^t | rho <= 64: never more than a few hundred trials.  All agree: q2 IS the
// division by this sd.  A power of two has S' = 1, yl = 0 and an exact product: proven, nothing to try.
//
// Exponents.  The trial runs at sd in [1, 2) and a in [2^52, 2^53); every operation scales exactly with
// the exponents of a and sd as long as nothing overflows or underflows, and sd itself is held to
// [2^-256, 2^256] so that yh and yl are normal.  A dividend whose quotient overflows gives inf or NaN in
// either form, and the forward pass clamps |q| by fmin(|q|, zcap) to the same finite zcap (without
// winsorising, zcap = inf, such a cell is -inf or about -1e308: no signal gets there).  A dividend so small
// that a yl or the quotient underflows gives a value below 2^-1000 in either form, far under the
// granularity of the z_shift it is subtracted from (the same note as on div_by_recip).
//
// Conservative by construction: not finite, not positive, subnormal, outside [2^-256, 2^256], or a
// significand of all ones (the reciprocal's rounding sits at a binade edge there; no model needs it): unproven.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

namespace div_const_proof {

enum { RHO_MAX = 64 };

inline double recip_low_host(double b, double yh) { return __builtin_fma(-b, yh, 1.0) * yh; }
inline double div_const2_host(double a, double yh, double yl)
{
    const double p = a * yl;
    return __builtin_fma(a, yh, p);
}

// 2^-n modulo the odd m (1 < m < 2^53): n halvings of 1, x -> x / 2 or (x + m) / 2
inline uint64_t inv_pow2_mod(int n, uint64_t m)
{
    uint64_t x = 1 % m;
    for (int i = 0; i < n; i++) x = (x & 1) ? (x + m) >> 1 : x >> 1;
    return x;
}

// 1: fma(a, yh, a * yl) == a / sd for every dividend (see above); 0: not shown
inline int proven(double sd)
{
    if (!(sd > 0.0) || !isfinite(sd)) return 0;
    uint64_t bits;
    memcpy(&bits, &sd, 8);
    const int ex = (int)(bits >> 52) & 0x7ff;
    if (ex == 0 || ex < 1023 - 256 || ex > 1023 + 256) return 0;
    const uint64_t frac = bits & 0xfffffffffffffull;
    if (frac == 0xfffffffffffffull) return 0;
    const uint64_t S = frac | (1ull << 52);
    int t = 0;
    while (!((S >> t) & 1)) t++;
    const uint64_t Sodd = S >> t;
    if (Sodd == 1) return 1;                                  // a power of two
    const double sdn = (double)S * 0x1p-52;                   // sd's significand in [1, 2)
    const double yh = 1.0 / sdn, yl = recip_low_host(sdn, yh);
    for (int k = 53; k <= 54; k++) {
        const uint64_t a_lo = k == 53 ? S : (1ull << 52), a_hi = k == 53 ? (1ull << 53) : S; // [a_lo, a_hi)
        const uint64_t inv = inv_pow2_mod(k - t, Sodd);
        for (int64_t rho = -RHO_MAX; rho <= RHO_MAX; rho++) {
            if (rho == 0 || (rho & (((int64_t)1 << t) - 1)) != 0) continue;
            int64_t r = (rho >> t) % (int64_t)Sodd;           // (2^t | rho: the shift is exact)
            if (r < 0) r += (int64_t)Sodd;
            uint64_t A = (uint64_t)(((unsigned __int128)(uint64_t)r * inv) % Sodd);
            if (A < a_lo) A += (a_lo - A + Sodd - 1) / Sodd * Sodd;
            for (; A < a_hi; A += Sodd) {
                const __int128 num = ((__int128)A << k) - rho; // = M S
                if (num % (__int128)S != 0) return 0;          // (cannot happen: the solver is wrong, prove nothing)
                const __int128 M = num / (__int128)S;
                if (!(M & 1)) continue;                        // an even M is a double, not a boundary
                const double a = (double)A;
                if (div_const2_host(a, yh, yl) != a / sdn) return 0;
            }
        }
    }
    return 1;
}

} // namespace div_const_proof
