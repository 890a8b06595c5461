"""Exact-arithmetic restatement of the question csrc/div_const_proof.h answers: is fma(a, yh, a * yl), with
yh = RN(1 / sd) and yl = RN(RN(1 - sd yh) yh), the IEEE quotient RN(a / sd) for EVERY double a?

Only dividends whose exact quotient lies within about 2^-104 of a rounding boundary can round differently.  With S, A
the 53-bit integer significands of sd and a, the boundaries of A / S are M / 2^k, M odd, k = 53 (A >= S) or 54
(A < S), and rho = 2^k A - M S measures the distance: the dividends with |rho| <= R are listed by solving
2^k A = rho (mod S) and tried one by one, every rounding done on fractions.Fraction.  Not a copy of the C++: Python
integers, pow(2, -n, m) for the inverse, float(Fraction) (correctly rounded in CPython) for RN."""
from fractions import Fraction
import math

R_DEFAULT = 64


def rn(x):
    """round-to-nearest-even of an exact rational to a double"""
    return float(x)


def fma(a, b, c):
    return rn(Fraction(a) * Fraction(b) + Fraction(c))


def recip_pair(sd):
    yh = rn(Fraction(1) / Fraction(sd))
    return yh, rn(Fraction(fma(-sd, yh, 1.0)) * Fraction(yh))


def two_op_quotient(a, sd):
    yh, yl = recip_pair(sd)
    return fma(a, yh, rn(Fraction(a) * Fraction(yl)))


def significand(x):
    m, e = math.frexp(x)
    return int(m * (1 << 53))


def candidates(sd, R=R_DEFAULT):
    """the integer significands A (2^52 <= A < 2^53) of the dividends whose quotient by sd lies within |rho| <= R of
    a rounding boundary; sd a positive normal double"""
    S = significand(sd)
    out = []
    for k, lo, hi in ((53, S, 1 << 53), (54, 1 << 52, S)):
        for rho in range(-R, R + 1):
            g = math.gcd(1 << k, S)
            if rho == 0 or rho % g:
                continue
            m = S // g
            if m == 1:
                continue                         # a power of two: every quotient is exact
            a0 = (rho // g) * pow((1 << k) // g, -1, m) % m
            A = a0 + (lo - a0 + m - 1) // m * m
            while A < hi:
                M, rem = divmod((A << k) - rho, S)
                assert rem == 0
                if M & 1:
                    out.append(A)
                A += m
    return out


def proven(sd, R=R_DEFAULT):
    """the verdict the library must give for sd"""
    if not (sd > 0.0) or math.isinf(sd) or sd < 2.0 ** -256 or sd > 2.0 ** 256:
        return False
    S = significand(sd)
    if S == (1 << 53) - 1:
        return False
    sdn = float(S) * 2.0 ** -52
    return all(two_op_quotient(float(A), sdn) == rn(Fraction(A) / Fraction(sdn)) for A in candidates(sdn, R))
