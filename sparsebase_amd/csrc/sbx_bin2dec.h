// sbx_bin2dec.h — exact binary floating point -> decimal text for the Matrix Market / edge-list writers.
//
// The mirror image of sbx_dec2bin.h.  A float or double bit pattern and a precision P in 1..17 give the characters
// printf("%.*g", P, (double)x) produces under glibc — which `ostream << x` prints at P = 6 (the reference writers,
// io/mtx_writer.cc and io/edge_list_writer.cc, use the stream's default precision; a float widens to double exactly).
// No floating-point arithmetic is involved: the exact value m * 2^e is scaled by 10^s in integers, s = P - 1 - X with
// X the decimal exponent, and rounded ONCE, half to even, to P significant digits:
//   s >= 0:  m * 5^s, shifted by e + s                  (the bits shifted out decide the rounding)
//   s <  0:  (m * 2^(e-j)) / 5^j, j = -s                (the remainder, and the bits shifted out, decide it)
// The fast path does this in 128-bit arithmetic (|s| small: the decimal exponents the values of real matrices have);
// the long path in multi-limb integers with the 5^k table every handle already holds (largest scale 323 + 17 = 340,
// the table reaches SBX_POW5_MAX = 400).  Its quotient is below 10^18: estimated from the top 128 / 64 bits of the
// operands and corrected by one multiply-compare.  The long path needs per-thread limb arrays, so on the device it is
// a kernel of its own over the few values that need it (sbx_text.hip); convert<false> never instantiates it.
// Compiles for the device (HIP) and for the host (g++: tests/test_bin2dec.py checks it against snprintf).
#pragma once
#include "sbx_dec2bin.h"

// What one value prints as, between the conversion and the write-out: the significant digits without trailing zeros
// as an integer, how many they are, and the decimal exponent of the first one.
enum : unsigned { SBX_DEC_FINITE = 0, SBX_DEC_ZERO = 1, SBX_DEC_INF = 2, SBX_DEC_NAN = 3, SBX_DEC_LONG = 4 };
struct sbx_decrec {
  uint64_t digits;
  int16_t exp10;
  uint8_t ndig;
  uint8_t kind;  // bit 0: sign; bits 1..: SBX_DEC_*
  uint32_t pad;
};

#define SBX_DEC_MAX_CHARS 24 /* -d.dddddddddddddddde-XXX */

namespace sbx_b2d {

SBX_HD uint64_t pow10_u64(int p, const uint64_t *pow5) {  // 10^p, p <= 19 (5^p is one limb up to p = 27)
  return pow5[(size_t)p * SBX_POW5_LIMBS] << p;
}

// 0 exact, 1 below half, 2 half, 3 above half: `r` against 2^(t-1), r < 2^t, 1 <= t <= 127
SBX_HD int cmp_half128(unsigned __int128 r, int t) {
  if (r == 0) return 0;
  const unsigned __int128 half = (unsigned __int128)1 << (t - 1);
  return r < half ? 1 : r == half ? 2 : 3;
}

// (hi * 2^64 + lo) / d with hi < d: quotient and remainder (Knuth D with 32-bit digits; Hacker's Delight divlu)
SBX_HD uint64_t div128by64(uint64_t hi, uint64_t lo, uint64_t d, uint64_t *rem) {
  const int s = sbx_d2b::clz64(d);
  d <<= s;
  if (s) {
    hi = (hi << s) | (lo >> (64 - s));
    lo <<= s;
  }
  const uint64_t b = 1ull << 32, d1 = d >> 32, d0 = d & 0xFFFFFFFFull, l1 = lo >> 32, l0 = lo & 0xFFFFFFFFull;
  uint64_t q1 = hi / d1, rh = hi - q1 * d1;
  while (q1 >= b || q1 * d0 > b * rh + l1) {
    q1--;
    rh += d1;
    if (rh >= b) break;
  }
  const uint64_t mid = hi * b + l1 - q1 * d;
  uint64_t q0 = mid / d1;
  rh = mid - q0 * d1;
  while (q0 >= b || q0 * d0 > b * rh + l0) {
    q0--;
    rh += d1;
    if (rh >= b) break;
  }
  *rem = (mid * b + l0 - q0 * d) >> s;
  return q1 * b + q0;
}

// floor(m * 2^e * 10^s) and what is left of it (0 exact, 1 below half, 2 half, 3 above half) in 128-bit arithmetic;
// false where the operands do not fit
SBX_HD bool scale_fast(uint64_t m, int e, int s, const uint64_t *pow5, uint64_t *q, int *cmp) {
  if (s >= 0) {
    if (s > 32) return false;  // m * 5^s < 2^53 * 2^74.4
    const uint64_t *p = pow5 + (size_t)s * SBX_POW5_LIMBS;
    const unsigned __int128 n = (unsigned __int128)m * p[0] + (((unsigned __int128)(m * p[1])) << 64);
    const int sh = e + s;
    if (sh >= 0) {
      if (sh >= 64 || (n >> (64 - sh)) != 0) return false;
      *q = (uint64_t)n << sh;
      *cmp = 0;
      return true;
    }
    const int t = -sh;
    if (t > 120) return false;
    const unsigned __int128 top = n >> t;
    if ((uint64_t)(top >> 64) != 0) return false;
    *q = (uint64_t)top;
    *cmp = cmp_half128(n & ((((unsigned __int128)1) << t) - 1), t);
    return true;
  }
  const int j = -s;
  if (j > 27) return false;  // 5^27 < 2^63
  const uint64_t p = pow5[(size_t)j * SBX_POW5_LIMBS];
  const int sh = e - j;
  uint64_t a, r1 = 0;
  int t = 0;
  if (sh >= 0) {
    if (sh >= 64 || (sh > 0 && (m >> (64 - sh)) != 0)) return false;
    a = m << sh;
  } else {
    t = -sh;
    if (t >= 63) return false;
    a = m >> t;
    r1 = m & ((1ull << t) - 1);
  }
  *q = a / p;
  const uint64_t r2 = a - *q * p;
  // the whole remainder is r2 * 2^t + r1, against 5^j * 2^t / 2 (5^j is odd)
  if (r2 == 0 && r1 == 0) *cmp = 0;
  else if (2 * r2 > p) *cmp = 3;
  else if (2 * r2 == p - 1) *cmp = t == 0 ? 1 : (r1 < (1ull << (t - 1)) ? 1 : r1 == (1ull << (t - 1)) ? 2 : 3);
  else *cmp = 1;
  return true;
}

// the same in multi-limb integers, for every finite value and every scale the table covers
SBX_HD void scale_long(uint64_t m, int e, int s, const uint64_t *pow5, uint64_t *q, int *cmp) {
  constexpr int NL = SBX_POW5_LIMBS + 2;
  if (s >= 0) {
    const uint64_t *p = pow5 + (size_t)s * SBX_POW5_LIMBS;
    uint64_t n[NL];
    unsigned __int128 carry = 0;
    for (int i = 0; i < SBX_POW5_LIMBS; i++) {
      const unsigned __int128 t = (unsigned __int128)p[i] * m + carry;
      n[i] = (uint64_t)t;
      carry = t >> 64;
    }
    n[SBX_POW5_LIMBS] = (uint64_t)carry;
    n[SBX_POW5_LIMBS + 1] = 0;
    const int sh = e + s;
    if (sh >= 0) {  // (an integer below 10^18: one limb)
      *q = sh < 64 ? n[0] << sh : 0;
      *cmp = 0;
      return;
    }
    const int t = -sh, limb = t >> 6, bit = t & 63;
    uint64_t v = 0;
    if (limb < NL) {
      v = n[limb] >> bit;
      if (bit && limb + 1 < NL) v |= n[limb + 1] << (64 - bit);
    }
    *q = v;
    // bit t - 1 is the half bit, everything below it sticky
    const int hb = t - 1, hl = hb >> 6;
    bool half = false, rest = false;
    for (int i = 0; i < NL; i++) {
      if (i < hl) rest |= n[i] != 0;
      else if (i == hl) {
        half = (n[i] >> (hb & 63)) & 1u;
        rest |= (n[i] & ((1ull << (hb & 63)) - 1ull)) != 0;
      }
    }
    *cmp = half ? (rest ? 3 : 2) : (rest ? 1 : 0);
    return;
  }
  const int j = -s;
  const uint64_t *b = pow5 + (size_t)j * SBX_POW5_LIMBS;
  const int bl = sbx_d2b::limbs_of(b, SBX_POW5_LIMBS);
  const int sh = e - j;
  uint64_t a[NL];
  uint64_t r1 = 0;
  int t = 0;
  const uint64_t m1[1] = {m};
  if (sh >= 0) {
    sbx_d2b::shl_multi(a, NL, m1, 1, sh);
  } else {
    t = -sh;
    for (int i = 0; i < NL; i++) a[i] = 0;
    a[0] = t < 64 ? m >> t : 0;
    r1 = t < 64 ? m & ((1ull << t) - 1) : m;
  }
  const int al = sbx_d2b::limbs_of(a, NL);
  // quotient (below 2^61) and remainder of a / b
  uint64_t quo = 0;
  uint64_t r2[NL];
  for (int i = 0; i < NL; i++) r2[i] = a[i];
  bool a_ge_b = al > bl;
  if (al == bl) {
    a_ge_b = true;
    for (int i = bl - 1; i >= 0; i--)
      if (a[i] != b[i]) { a_ge_b = a[i] > b[i]; break; }
  }
  if (a_ge_b) {
    const int bbits = 64 * bl - sbx_d2b::clz64(b[bl - 1]);
    uint64_t rem;
    if (bbits <= 64) {
      quo = div128by64(a[1], a[0], b[0], &rem);
    } else {
      // top 64 bits of b, the bits of a from the same position on: a / b lies in (at / (bt + 1), at / bt]
      const int shn = bbits - 64, limb = shn >> 6, bit = shn & 63;
      auto word = [&](const uint64_t *x, int nx, int i) -> uint64_t {
        uint64_t v = i < nx ? x[i] >> bit : 0;
        if (bit && i + 1 < nx) v |= x[i + 1] << (64 - bit);
        return v;
      };
      const uint64_t bt = word(b, SBX_POW5_LIMBS, limb);
      const uint64_t at_lo = word(a, NL, limb), at_hi = word(a, NL, limb + 1);
      quo = at_hi >= bt ? ~0ull : div128by64(at_hi, at_lo, bt, &rem);
    }
    // r2 = a - quo * b, one step back where the estimate was one too large
    for (int round = 0; round < 3; round++) {
      uint64_t prod[NL];
      unsigned __int128 carry = 0;
      for (int i = 0; i < NL; i++) {
        const unsigned __int128 x = (unsigned __int128)(i < SBX_POW5_LIMBS ? b[i] : 0) * quo + carry;
        prod[i] = (uint64_t)x;
        carry = x >> 64;
      }
      bool gt = false;
      for (int i = NL - 1; i >= 0; i--)
        if (prod[i] != a[i]) { gt = prod[i] > a[i]; break; }
      if (gt) { quo--; continue; }
      uint64_t borrow = 0;
      for (int i = 0; i < NL; i++) {
        const uint64_t d = a[i] - prod[i] - borrow;
        borrow = (a[i] < prod[i] || (a[i] == prod[i] && borrow)) ? 1u : 0u;
        r2[i] = d;
      }
      break;
    }
  }
  *q = quo;
  // the whole remainder is r2 * 2^t + r1 against b * 2^t / 2, b odd: compare 2 * r2 with b
  bool r2_zero = true;
  for (int i = 0; i < NL; i++) r2_zero &= r2[i] == 0;
  if (r2_zero && r1 == 0) { *cmp = 0; return; }
  uint64_t tw[NL];
  for (int i = NL - 1; i > 0; i--) tw[i] = (r2[i] << 1) | (r2[i - 1] >> 63);
  tw[0] = r2[0] << 1;
  bool gt = false, eq = true;
  for (int i = NL - 1; i >= 0; i--) {
    const uint64_t bi = i < SBX_POW5_LIMBS ? b[i] : 0;
    if (tw[i] != bi) { gt = tw[i] > bi; eq = false; break; }
  }
  (void)eq;  // (b is odd, 2 * r2 even)
  if (gt) { *cmp = 3; return; }
  // b - 2 * r2 == 1 ?
  uint64_t borrow = 0;
  bool is_one = true;
  for (int i = 0; i < NL; i++) {
    const uint64_t bi = i < SBX_POW5_LIMBS ? b[i] : 0;
    const uint64_t d = bi - tw[i] - borrow;
    borrow = (bi < tw[i] || (bi == tw[i] && borrow)) ? 1u : 0u;
    is_one &= d == (i == 0 ? 1u : 0u);
  }
  if (!is_one || t == 0) { *cmp = 1; return; }
  if (t > 64) { *cmp = 1; return; }  // r1 = m < 2^53 < 2^(t-1)
  const uint64_t half = 1ull << (t - 1);
  *cmp = r1 < half ? 1 : r1 == half ? 2 : 3;
}

// m * 2^e (m != 0, below 2^53) rounded to P significant digits: the digits as an integer in [10^(P-1), 10^P) and the
// decimal exponent of the first one.  LONG = false: false is returned where the fast path does not reach.
template <bool LONG>
SBX_HD bool convert(uint64_t m, int e, int P, const uint64_t *pow5, uint64_t *digits, int *exp10) {
  const int b = 64 - sbx_d2b::clz64(m) + e;  // 2^(b-1) <= value < 2^b
  int k = ((b - 1) * 315653) >> 20;          // floor((b-1) * log10(2)), at most one off the decimal exponent
  const uint64_t lo10 = pow10_u64(P - 1, pow5), hi10 = pow10_u64(P, pow5);
  uint64_t q = 0;
  int cmp = 0;
  for (int tries = 0; tries < 4; tries++) {
    const int s = P - 1 - k;
    if (!scale_fast(m, e, s, pow5, &q, &cmp)) {
      if constexpr (LONG) scale_long(m, e, s, pow5, &q, &cmp);
      else return false;
    }
    if (q >= hi10) k++;
    else if (q < lo10) k--;
    else break;
  }
  if (cmp == 3 || (cmp == 2 && (q & 1u))) q++;
  if (q == hi10) {
    q = lo10;
    k++;
  }
  *digits = q;
  *exp10 = k;
  return true;
}

SBX_HD sbx_decrec make_rec(unsigned kind, bool neg) {
  sbx_decrec r;
  r.digits = 0; r.exp10 = 0; r.ndig = 0; r.kind = (uint8_t)((kind << 1) | (neg ? 1u : 0u)); r.pad = 0;
  return r;
}

// IEEE fields -> record.  BITS 64 / 32.  LONG = false leaves the values the fast path does not reach as SBX_DEC_LONG.
template <bool LONG, int BITS>
SBX_HD sbx_decrec to_record(uint64_t bits, int P, const uint64_t *pow5) {
  constexpr int MB = BITS == 64 ? 52 : 23, EMAX = BITS == 64 ? 0x7FF : 0xFF, BIAS = BITS == 64 ? 1075 : 150;
  const bool neg = (bits >> (BITS - 1)) & 1u;
  const int ex = (int)((bits >> MB) & (uint64_t)EMAX);
  const uint64_t frac = bits & ((1ull << MB) - 1ull);
  if (ex == EMAX) return make_rec(frac ? SBX_DEC_NAN : SBX_DEC_INF, neg);
  if (ex == 0 && frac == 0) return make_rec(SBX_DEC_ZERO, neg);
  const uint64_t m = ex == 0 ? frac : frac | (1ull << MB);
  const int e = (ex == 0 ? 1 : ex) - BIAS;
  uint64_t q;
  int x;
  if (!convert<LONG>(m, e, P, pow5, &q, &x)) return make_rec(SBX_DEC_LONG, neg);
  int nd = P;  // trailing zeros go: %g strips them
  if (nd > 8 && q % 100000000ull == 0) { q /= 100000000ull; nd -= 8; }
  if (nd > 4 && q % 10000u == 0) { q /= 10000u; nd -= 4; }
  if (nd > 2 && q % 100u == 0) { q /= 100u; nd -= 2; }
  if (nd > 1 && q % 10u == 0) { q /= 10u; nd -= 1; }
  if (nd > 8 && q % 100000000ull == 0) { q /= 100000000ull; nd -= 8; }  // (16 zeros: 8 + 4 + 2 + 1 + 1)
  if (nd > 1 && q % 10u == 0) { q /= 10u; nd -= 1; }
  sbx_decrec r = make_rec(SBX_DEC_FINITE, neg);
  r.digits = q;
  r.exp10 = (int16_t)x;
  r.ndig = (uint8_t)nd;
  return r;
}

// characters the record prints as under "%.*g" with precision P
SBX_HD int text_length(const sbx_decrec &r, int P) {
  const int neg = r.kind & 1u;
  const unsigned kind = r.kind >> 1;
  if (kind == SBX_DEC_ZERO) return 1 + neg;
  if (kind != SBX_DEC_FINITE) return 3 + neg;
  const int x = r.exp10, nd = r.ndig;
  if (x >= -4 && x < P) {
    if (x >= 0) return neg + (nd > x + 1 ? nd + 1 : x + 1);
    return neg + nd + 1 - x;
  }
  const int ax = x < 0 ? -x : x;
  return neg + nd + (nd > 1 ? 1 : 0) + 2 + (ax >= 100 ? 3 : 2);
}

// unsigned decimal, most significant digit first; returns the number of characters
SBX_HD int emit_u64(uint64_t v, char *dst) {
  int nd = 1;
  if (v >> 32) {
    for (uint64_t t = v; t >= 10; t /= 10) nd++;
    for (int i = nd - 1; i >= 0; i--) {
      dst[i] = (char)('0' + (int)(v % 10));
      v /= 10;
    }
    return nd;
  }
  uint32_t w = (uint32_t)v;
  for (uint32_t t = w; t >= 10; t /= 10) nd++;
  for (int i = nd - 1; i >= 0; i--) {
    dst[i] = (char)('0' + (int)(w % 10));
    w /= 10;
  }
  return nd;
}
SBX_HD int length_u64(uint64_t v) {
  int nd = 1;
  if (v >> 32) {
    for (uint64_t t = v; t >= 10; t /= 10) nd++;
    return nd;
  }
  for (uint32_t t = (uint32_t)v; t >= 10; t /= 10) nd++;
  return nd;
}

// writes text_length(r, P) characters at dst
SBX_HD int emit(const sbx_decrec &r, int P, char *dst) {
  int o = 0;
  if (r.kind & 1u) dst[o++] = '-';
  const unsigned kind = r.kind >> 1;
  if (kind == SBX_DEC_ZERO) { dst[o++] = '0'; return o; }
  if (kind == SBX_DEC_INF) { dst[o] = 'i'; dst[o + 1] = 'n'; dst[o + 2] = 'f'; return o + 3; }
  if (kind != SBX_DEC_FINITE) { dst[o] = 'n'; dst[o + 1] = 'a'; dst[o + 2] = 'n'; return o + 3; }
  const int x = r.exp10, nd = r.ndig;
  const bool fixed = x >= -4 && x < P;
  // digit i (0: the first) goes to lead + i, one further behind the point
  int lead = o, point_after = 0x7FFF, end;
  if (fixed && x < 0) {
    dst[o] = '0';
    dst[o + 1] = '.';
    for (int i = 0; i < -x - 1; i++) dst[o + 2 + i] = '0';
    lead = o + 1 - x;
    end = lead + nd;
  } else if (fixed) {
    if (nd > x + 1) {
      point_after = x;
      dst[o + x + 1] = '.';
      end = o + nd + 1;
    } else {
      for (int i = nd; i < x + 1; i++) dst[o + i] = '0';
      end = o + x + 1;
    }
  } else {
    if (nd > 1) {
      point_after = 0;
      dst[o + 1] = '.';
    }
    end = o + nd + (nd > 1 ? 1 : 0);
  }
  uint32_t lo9 = (uint32_t)(r.digits % 1000000000ull), hi = (uint32_t)(r.digits / 1000000000ull);
  for (int c = 0; c < nd; c++) {
    const int i = nd - 1 - c;
    uint32_t d;
    if (c < 9) { d = lo9 % 10u; lo9 /= 10u; }
    else { d = hi % 10u; hi /= 10u; }
    dst[lead + i + (i > point_after ? 1 : 0)] = (char)('0' + (int)d);
  }
  if (!fixed) {
    const int ax = x < 0 ? -x : x;
    dst[end++] = 'e';
    dst[end++] = x < 0 ? '-' : '+';
    if (ax >= 100) dst[end++] = (char)('0' + ax / 100);
    dst[end++] = (char)('0' + (ax / 10) % 10);
    dst[end++] = (char)('0' + ax % 10);
  }
  return end;
}

}  // namespace sbx_b2d

// "%.*g" of a double / float bit pattern into dst (at most SBX_DEC_MAX_CHARS characters, no terminator); the length
SBX_HD int sbx_format_double_bits(uint64_t bits, int precision, const uint64_t *pow5, char *dst) {
  const sbx_decrec r = sbx_b2d::to_record<true, 64>(bits, precision, pow5);
  return sbx_b2d::emit(r, precision, dst);
}
SBX_HD int sbx_format_float_bits(uint32_t bits, int precision, const uint64_t *pow5, char *dst) {
  const sbx_decrec r = sbx_b2d::to_record<true, 32>(bits, precision, pow5);
  return sbx_b2d::emit(r, precision, dst);
}
