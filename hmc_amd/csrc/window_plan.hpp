// window_plan.hpp — the configurations of hmc_window_phasings (exact_query.hip,
// exact_window_phasings): for one individual and one window of loci, which loci
// branch, how many ordered configurations there are, and the map between a
// configuration code and the two allele strings it spells.  Free of the context
// so that the host sanitizer program (tests/sanitize/window_main.cpp) can drive
// it; the digit functions are the kernel's too (HMC_WIN_HD).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define HMC_WIN_HD __host__ __device__
#else
#define HMC_WIN_HD
#endif

namespace hmc {

constexpr int WIN_K_MAX = 1024;       // rows per (individual, window)
constexpr int WIN_CAP_MAX = 1024;     // ordered configurations the widest kernel holds, and the default cap
constexpr int WIN_DIGITS_MAX = 10;    // branching loci of a window within the cap (every radix is at least 2)
constexpr uint8_t WIN_MISSING = 0xFF; // a missing input allele (MISSING, hmc_internal.hpp)

// A branching locus of a window — heterozygous, or an input allele missing —
// is one digit of the configuration code.  Its values are the ordered allele
// pairs (a side, b side) the genotype allows, numbered in lexicographic order:
//   WIN_HET   alleles x < y:                 (x, y), (y, x)                 radix 2
//   WIN_ONE   allele x known, y alleles:     (z, x) z < x; (x, z); (z, x) z > x   radix 2 y - 1
//   WIN_BOTH  y alleles at the locus:        (z, w) = z y + w               radix y^2
// The code takes the window's branching loci as digits, the first locus most
// significant, so codes ascend as (a0, b0, a1, b1, ...) does.
enum : uint8_t { WIN_HET = 0, WIN_ONE = 1, WIN_BOTH = 2 };
struct WinDigit {
  int32_t rel;  // the locus, counted from the window's start
  uint8_t kind, x, y, pad;
};

HMC_WIN_HD inline int win_radix(const WinDigit &g) {
  return g.kind == WIN_HET ? 2 : g.kind == WIN_ONE ? 2 * (int)g.y - 1 : (int)g.y * (int)g.y;
}
// the digit of the ordered pair (xa, xb), or -1 when the genotype does not allow it
HMC_WIN_HD inline int win_encode(const WinDigit &g, uint32_t xa, uint32_t xb) {
  const uint32_t x = g.x, y = g.y;
  if (g.kind == WIN_HET) return xa == x && xb == y ? 0 : xa == y && xb == x ? 1 : -1;
  if (g.kind == WIN_ONE) {
    if (xa >= y || xb >= y) return -1;
    if (xa == x) return (int)(x + xb);
    if (xb != x) return -1;
    return xa < x ? (int)xa : (int)(y + xa - 1);
  }
  return xa < y && xb < y ? (int)(xa * y + xb) : -1;
}
HMC_WIN_HD inline void win_decode(const WinDigit &g, int d, uint32_t &xa, uint32_t &xb) {
  const int x = g.x, y = g.y;
  if (g.kind == WIN_HET) {
    xa = d ? y : x;
    xb = d ? x : y;
  } else if (g.kind == WIN_ONE) {
    if (d < x) {
      xa = d;
      xb = x;
    } else if (d < x + y) {
      xa = x;
      xb = d - x;
    } else {
      xa = d - y + 1;
      xb = x;
    }
  } else {
    xa = d / y;
    xb = d % y;
  }
}
HMC_WIN_HD inline int win_swap_digit(const WinDigit &g, int d) {
  uint32_t xa, xb;
  win_decode(g, d, xa, xb);
  return win_encode(g, xb, xa);
}

// The configuration with the two sides exchanged, over the first nd digits.
HMC_WIN_HD inline int win_swap_code(const WinDigit *g, int nd, int code) {
  int out = 0, mult = 1;
  for (int i = nd - 1; i >= 0; --i) {
    const int r = win_radix(g[i]);
    out += win_swap_digit(g[i], code % r) * mult;
    code /= r;
    mult *= r;
  }
  return out;
}
// digit i (0 the first branching locus) of a code of nd digits
HMC_WIN_HD inline int win_digit_of(const WinDigit *g, int nd, int code, int i) {
  for (int q = nd - 1; q > i; --q) code /= win_radix(g[q]);
  return code % win_radix(g[i]);
}
// A row spells the unordered pair once: the orientation whose a side is the
// lexicographically smaller string, which is the smaller of the two codes.
HMC_WIN_HD inline bool win_canonical(const WinDigit *g, int nd, int code) { return code <= win_swap_code(g, nd, code); }
// The canonical order of rows of equal probability: the a-side string, then the
// b-side string, by allele index (fixed loci are equal in every row).
HMC_WIN_HD inline bool win_order_less(const WinDigit *g, int nd, int c, int d) {
  for (int side = 0; side < 2; ++side)
    for (int i = 0; i < nd; ++i) {
      uint32_t ca, cb, da, db;
      win_decode(g[i], win_digit_of(g, nd, c, i), ca, cb);
      win_decode(g[i], win_digit_of(g, nd, d, i), da, db);
      const uint32_t u = side ? cb : ca, v = side ? db : da;
      if (u != v) return u < v;
    }
  return false;
}

// One (individual, window): its digits are dig[dig0 .. dig0 + nd); C ordered
// configurations, 0 when they exceed the cap (status 4: no digits kept).
struct WinItem {
  uint32_t dig0;
  int32_t nd, C;
};

// The branching loci of the window g0[0 .. len), g1[0 .. len) (allele-table
// indices, WIN_MISSING = missing) with nall[k] alleles at locus k, appended to
// `dig` when the product of their radices is at most cap (<= WIN_CAP_MAX).
// Returns the product, or cap + 1 as soon as it exceeds the cap.
inline long long win_plan(const uint8_t *g0, const uint8_t *g1, const uint8_t *nall, int len, int cap, std::vector<WinDigit> &dig) {
  const size_t keep = dig.size();
  long long C = 1;
  for (int k = 0; k < len; ++k) {
    const uint8_t a = g0[k], b = g1[k];
    if (a != WIN_MISSING && b != WIN_MISSING && a == b) continue;  // fixed
    WinDigit g{k, 0, 0, 0, 0};
    if (a != WIN_MISSING && b != WIN_MISSING) {
      g.kind = WIN_HET;
      g.x = a < b ? a : b;
      g.y = a < b ? b : a;
    } else if (a == WIN_MISSING && b == WIN_MISSING) {
      g.kind = WIN_BOTH;
      g.y = nall[k];
    } else {
      g.kind = WIN_ONE;
      g.x = a == WIN_MISSING ? b : a;
      g.y = nall[k];
    }
    C *= win_radix(g);
    if (C > cap) {
      dig.resize(keep);
      return (long long)cap + 1;
    }
    if (win_radix(g) > 1) dig.push_back(g);  // (a locus of one allele branches nowhere)
  }
  return C;
}

// The two allele strings of a code over the window: fixed loci from the
// genotype, branching loci from the digits.  xa, xb: [len] allele indices.
inline void win_spell(const WinDigit *g, int nd, int code, const uint8_t *g0, const uint8_t *g1, int len, uint8_t *xa,
                      uint8_t *xb) {
  // (a locus with a missing allele and a single allele in its table is fixed too: allele 0)
  for (int k = 0; k < len; ++k) xa[k] = xb[k] = g0[k] != WIN_MISSING ? g0[k] : g1[k] != WIN_MISSING ? g1[k] : (uint8_t)0;
  for (int i = nd - 1; i >= 0; --i) {
    const int r = win_radix(g[i]);
    uint32_t a, b;
    win_decode(g[i], code % r, a, b);
    code /= r;
    xa[g[i].rel] = (uint8_t)a;
    xb[g[i].rel] = (uint8_t)b;
  }
}
// The code of two allele strings, or -1 when the genotype does not allow them.
inline int win_code_of(const WinDigit *g, int nd, const uint8_t *xa, const uint8_t *xb) {
  int code = 0;
  for (int i = 0; i < nd; ++i) {
    const int d = win_encode(g[i], xa[g[i].rel], xb[g[i].rel]);
    if (d < 0) return -1;
    code = code * win_radix(g[i]) + d;
  }
  return code;
}

}  // namespace hmc
