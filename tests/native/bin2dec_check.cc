// CPU unit test of sparsebase_amd/csrc/sbx_bin2dec.h against snprintf("%.*g") (test infrastructure).
// usage: bin2dec_check <count> <seed>    prints "ok <doubles> <floats>" (inputs, each at every precision 1..17) or
// the first mismatches
#include <cfloat>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "sbx_bin2dec.h"

static std::vector<uint64_t> table((size_t)SBX_TABLE_WORDS);
static long bad = 0, n_double = 0, n_float = 0;

// where the 128-bit path applies, the multi-limb path must give the same quotient and the same remainder class
static void check_paths(uint64_t m, int e) {
  const int b = 64 - __builtin_clzll(m) + e;
  const int k = ((b - 1) * 315653) >> 20;
  for (int p = 1; p <= 17; p++)
    for (int dk = -1; dk <= 1; dk++) {
      const int s = p - 1 - (k + dk);
      uint64_t qf, ql;
      int cf, cl;
      if (!sbx_b2d::scale_fast(m, e, s, table.data(), &qf, &cf)) continue;
      sbx_b2d::scale_long(m, e, s, table.data(), &ql, &cl);
      if (qf != ql || cf != cl) {
        if (bad < 10) std::printf("PATHS m=%" PRIu64 " e=%d s=%d: fast %" PRIu64 "/%d long %" PRIu64 "/%d\n", m, e, s, qf, cf, ql, cl);
        bad++;
      }
    }
}

static void check_double(double x) {
  uint64_t bits;
  memcpy(&bits, &x, 8);
  n_double++;
  if (std::isfinite(x) && x != 0.0) {
    const int ex = (int)((bits >> 52) & 0x7FF);
    const uint64_t frac = bits & ((1ull << 52) - 1);
    check_paths(ex ? frac | (1ull << 52) : frac, (ex ? ex : 1) - 1075);
  }
  for (int p = 1; p <= 17; p++) {
    char want[64], got[64];
    const int wl = snprintf(want, sizeof want, "%.*g", p, x);
    const int gl = sbx_format_double_bits(bits, p, table.data(), got);
    if (gl != wl || memcmp(got, want, (size_t)wl) != 0) {
      if (bad < 10) std::printf("MISMATCH double %016" PRIx64 " P=%d: got %.*s want %s\n", bits, p, gl, got, want);
      bad++;
    }
  }
}

static void check_float(float x) {
  uint32_t bits;
  memcpy(&bits, &x, 4);
  n_float++;
  for (int p = 1; p <= 17; p++) {
    char want[64], got[64];
    const int wl = snprintf(want, sizeof want, "%.*g", p, (double)x);
    const int gl = sbx_format_float_bits(bits, p, table.data(), got);
    if (gl != wl || memcmp(got, want, (size_t)wl) != 0) {
      if (bad < 10) std::printf("MISMATCH float %08x P=%d: got %.*s want %s\n", bits, p, gl, got, want);
      bad++;
    }
  }
}

static void both(double x) {
  check_double(x);
  check_double(-x);
  check_float((float)x);  // (whatever float the double rounds to: inf and 0 included)
  check_float(-(float)x);
}

int main(int argc, char **argv) {
  const long count = argc > 1 ? atol(argv[1]) : 100000;
  std::mt19937_64 g(argc > 2 ? atoll(argv[2]) : 1);
  sbx_pow5_table_fill(table.data());

  // the fixed inputs: zeros, the ends of both ranges, the ties of the issue's text, every power of two and of ten
  const double fixed[] = {0.0, 1.0, 0.5, 2.5, 1.5, 3.5, 0.25, 0.125, 0.375, 1000005.0, 1000015.0, 999999.5, 999998.5, 9999995.0,
                          9.5, 99.5, 0.1, 0.3, 1e23, 8.5e22, 123456.5, 123455.5, 1e-5, 1e-4, 0.0001234565, 100000.0, 1e6,
                          999999.0, 9999999.0, 1e16, 1e17, 99999999999999992.0, 4.35, 0.95, 9.95, 0.00095, 5e-324,
                          DBL_MIN, DBL_MAX, 2.2250738585072009e-308 /* largest subnormal */, (double)FLT_MAX, (double)FLT_MIN,
                          1.4012984643248171e-45, 1.1754942106924411e-38 /* largest float subnormal */, 1.7976931348623157e308,
                          INFINITY, NAN};
  for (double x : fixed) both(x);
  for (int e = -1074; e <= 1023; e++) {
    both(std::ldexp(1.0, e));
    both(std::ldexp(3.0, e > -1074 ? e - 1 : e));
  }
  for (int e = -324; e <= 308; e++) {
    char buf[32];
    snprintf(buf, sizeof buf, "1e%d", e);
    both(strtod(buf, nullptr));
    snprintf(buf, sizeof buf, "9.9999999999999995e%d", e);
    both(strtod(buf, nullptr));
  }
  // NaNs of both signs with payloads
  for (uint64_t payload : {1ull, 0x8000000000000ull, 0xFFFFFFFFFFFFFull}) {
    for (uint64_t sign : {0ull, 1ull}) {
      const uint64_t bits = (sign << 63) | (0x7FFull << 52) | payload;
      double x;
      memcpy(&x, &bits, 8);
      check_double(x);
      const uint32_t fb = (uint32_t)(sign << 31) | (0xFFu << 23) | (uint32_t)(payload & 0x7FFFFFu) | 1u;
      float f;
      memcpy(&f, &fb, 4);
      check_float(f);
    }
  }

  for (long i = 0; i < count; i++) {
    // (1) uniformly random bit patterns: subnormals, inf and NaN of both signs included
    {
      const uint64_t bits = g();
      double x;
      memcpy(&x, &bits, 8);
      check_double(x);
      const uint32_t fb = (uint32_t)g();
      float f;
      memcpy(&f, &fb, 4);
      check_float(f);
    }
    const int kind = (int)(g() % 4);
    if (kind == 0) {  // short decimals k / 10^j
      const int j = (int)(g() % 12);
      const double x = (double)(int64_t)(g() % 2000000) / std::pow(10.0, j);
      both(x);
    } else if (kind == 1) {  // exact ties at the P-th digit: I + 1/2, I + odd/2^t (every precision is checked)
      const int d = 1 + (int)(g() % 15);
      uint64_t lim = 1;
      for (int k = 0; k < d; k++) lim *= 10;
      const uint64_t I = lim / 10 + g() % (lim - lim / 10);
      const int t = 1 + (int)(g() % 4);
      const double x = (double)I + (double)(2 * (g() % (1u << (t - 1))) + 1) / (double)(1u << t);
      both(x);
      both(x + 1.0);  // the odd / even neighbour
    } else if (kind == 2) {  // integer ties: (10 I + 5) * 10^z below 2^53, and their neighbours
      const int d = 1 + (int)(g() % 10);
      uint64_t lim = 1;
      for (int k = 0; k < d; k++) lim *= 10;
      const uint64_t I = lim / 10 + g() % (lim - lim / 10);
      uint64_t v = 10 * I + 5;
      for (int z = (int)(g() % 4); z > 0; z--) v *= 10;
      both((double)v);
      both((double)(v + 10));
      both(std::nextafter((double)v, 0.0));
      both(std::nextafter((double)v, INFINITY));
    } else {  // matrix-like magnitudes with full mantissas
      const double x = std::ldexp((double)(g() % (1ull << 53)), -53) * std::pow(10.0, (double)((int)(g() % 24) - 12));
      both(x);
    }
  }
  if (bad) {
    std::printf("FAILED %ld mismatches (%ld doubles, %ld floats)\n", bad, n_double, n_float);
    return 1;
  }
  std::printf("ok %ld %ld\n", n_double, n_float);
  return 0;
}
