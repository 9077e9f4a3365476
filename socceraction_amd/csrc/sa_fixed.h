// The fixed-point format of the order-independent grouped sums (sa_group.hip).
//
// A finite double v of a column with scale exponent E (contract |v| < 2^E) becomes the integer
//     Q = trunc(v * 2^(95 - E))            (toward zero, |Q| < 2^95)
// taken exactly from v's mantissa and exponent bits: no floating-point operation is involved.
// Q is split into three limbs of 32 magnitude bits, Q = s * (m2 * 2^64 + m1 * 2^32 + m0), and
// each limb, carrying the sign s of v, is summed in an int64 of its own.  Fewer than 2^30 rows
// per table keep every limb sum inside int64.  Integer addition is associative, so the three sums
// of a group do not depend on the order, the chunking or the number of devices they were added
// in.  sa_fx_finalize rounds the exact total S = sum(m2) * 2^64 + sum(m1) * 2^32 + sum(m0) ONCE,
// to the nearest double (ties to even), and scales it by 2^(E - 95).
//
// Plain C++ for the host (scripts/fixed_sum_host.cc) and __host__ __device__ under hipcc.
#pragma once

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define SA_FX_HD __host__ __device__
#else
#define SA_FX_HD
#endif

#define SA_FX_FRAC_BITS 95    /* Q = trunc(v * 2^(SA_FX_FRAC_BITS - E)) */
#define SA_FX_EXP_MIN (-900)  /* scale exponents a column may carry */
#define SA_FX_EXP_MAX 900
#define SA_FX_MAX_ROWS (1 << 30) /* fewer rows than this per table: limb sums fit int64 */

// what sa_fx_quantize returns
#define SA_FX_OK 0
#define SA_FX_NAN 1        /* adds nothing (pandas' sum skips NaN) */
#define SA_FX_NONFINITE 2  /* +-inf */
#define SA_FX_RANGE 4      /* |v| >= 2^E */

SA_FX_HD inline uint64_t sa_fx_bits(double v) {
  uint64_t b;
  __builtin_memcpy(&b, &v, sizeof(b));
  return b;
}

// What sa_fx_quantize(v, E, ...) would return, without the limbs.
SA_FX_HD inline int sa_fx_classify(double v, int E) {
  const uint64_t b = sa_fx_bits(v);
  const int e = (int)((b >> 52) & 0x7FF);
  if (e == 0x7FF) return (b & 0xFFFFFFFFFFFFFull) ? SA_FX_NAN : SA_FX_NONFINITE;
  return e - 1022 > E ? SA_FX_RANGE : SA_FX_OK;
}

// The limbs of v at scale exponent E: m[0..2] (magnitudes) and *neg (the sign they carry).
// Returns SA_FX_OK, or the reason the value adds nothing (m = 0 then).  -0.0 and magnitudes
// below the resolution 2^(E - 95) give m = 0, SA_FX_OK.
SA_FX_HD inline int sa_fx_quantize(double v, int E, uint32_t m[3], int* neg) {
  const uint64_t b = sa_fx_bits(v);
  const int e = (int)((b >> 52) & 0x7FF);
  const uint64_t frac = b & 0xFFFFFFFFFFFFFull;
  *neg = (int)(b >> 63);
  m[0] = m[1] = m[2] = 0;
  if (e == 0x7FF) return frac ? SA_FX_NAN : SA_FX_NONFINITE;
  // |v| = M * 2^ex, M < 2^53 (normal: bit 52 set)
  const uint64_t M = e ? (frac | (1ull << 52)) : frac;
  const int ex = (e ? e : 1) - 1075;
  if (e && e - 1022 > E) return SA_FX_RANGE;  // 2^(e - 1023) <= |v|: in range iff e - 1023 < E
  const int sh = ex + SA_FX_FRAC_BITS - E;     // Q = M * 2^sh truncated; sh <= 42 in range
  uint64_t lo, hi;
  if (sh >= 0) {
    lo = M << sh;
    hi = sh ? (M >> (64 - sh)) : 0;
  } else {
    lo = sh > -64 ? (M >> -sh) : 0;
    hi = 0;
  }
  m[0] = (uint32_t)lo;
  m[1] = (uint32_t)(lo >> 32);
  m[2] = (uint32_t)hi;
  if (!(m[0] | m[1] | m[2])) *neg = 0;
  return SA_FX_OK;
}

SA_FX_HD inline int sa_fx_clz64(uint64_t x) {  // x != 0
  int n = 0;
  if (!(x >> 32)) { n += 32; x <<= 32; }
  if (!(x >> 48)) { n += 16; x <<= 16; }
  if (!(x >> 56)) { n += 8; x <<= 8; }
  if (!(x >> 60)) { n += 4; x <<= 4; }
  if (!(x >> 62)) { n += 2; x <<= 2; }
  if (!(x >> 63)) { n += 1; }
  return n;
}

// (s2 * 2^64 + s1 * 2^32 + s0) * 2^(E - 95), rounded once to the nearest double, ties to even.
// Each limb sum is below 2^62 in magnitude (SA_FX_MAX_ROWS), so the total fits 128 signed bits.
SA_FX_HD inline double sa_fx_finalize(int64_t s0, int64_t s1, int64_t s2, int E) {
  // the total as a signed 128-bit integer (hi, lo)
  uint64_t lo = (uint64_t)s0;
  int64_t hi = s0 < 0 ? -1 : 0;
  const uint64_t add = (uint64_t)s1 << 32;
  lo += add;
  hi += (s1 >> 32) + (lo < add ? 1 : 0);  // arithmetic shift: the high part of s1 * 2^32
  hi += s2;
  const int negative = hi < 0;
  uint64_t mh = (uint64_t)hi, ml = lo;
  if (negative) {  // magnitude
    ml = ~ml + 1;
    mh = ~mh + (ml == 0 ? 1 : 0);
  }
  if (!(mh | ml)) return 0.0;
  const int lz = mh ? sa_fx_clz64(mh) : 64 + sa_fx_clz64(ml);
  const int nbits = 128 - lz;  // the leading one is bit nbits - 1
  uint64_t mant;               // 53 bits, bit 52 set
  if (nbits <= 53) {
    mant = ml << (53 - nbits);  // exact
  } else {
    const int shift = nbits - 53;  // 1..75: bits below `shift` are dropped
    uint64_t guard, sticky;
    if (shift < 64) {
      mant = (ml >> shift) | (mh << (64 - shift));  // shift >= 1
      guard = (ml >> (shift - 1)) & 1;
      sticky = shift > 1 ? (ml << (65 - shift)) : 0;
    } else {
      const int s = shift - 64;  // 0..11
      mant = mh >> s;
      guard = s ? (mh >> (s - 1)) & 1 : (ml >> 63);
      sticky = s ? ((s > 1 ? (mh << (65 - s)) : 0) | ml) : (ml << 1);
    }
    mant &= (1ull << 53) - 1;
    if (guard && (sticky || (mant & 1))) ++mant;  // round half to even
  }
  int p = nbits - 53 + E - SA_FX_FRAC_BITS;  // value = mant * 2^p
  if (mant >> 53) {                           // the round-up carried out of 53 bits
    mant >>= 1;
    ++p;
  }
  // E in [-900, 900] keeps the result a normal double: biased exponent in [28, 1954]
  const uint64_t bits = ((uint64_t)negative << 63) | ((uint64_t)(p + 52 + 1023) << 52) | (mant & ((1ull << 52) - 1));
  double out;
  __builtin_memcpy(&out, &bits, sizeof(out));
  return out;
}
