// Text formatting shared by the device renderer (render.hip) and its host-side test shim (tests/render_fmt_shim.cpp).
//
// fmt_fixed() prints a double exactly as CPython's '%.Nf' % x does for N = 1, 2, 3: the exact binary value is rounded half
// to even at the N-th decimal (2.675 -> "2.67", 0.125 -> "0.12"), and a negative value keeps its sign when it rounds to
// zero ("-0.00").  Integer arithmetic on the mantissa and exponent only: the 53-bit mantissa times 10^3 fits in 64 bits.
// No floating division, no printf.  A value that cannot occur in the writers' fields (non-finite, |x| >= 2^53) prints
// as "0" followed by the decimals and returns false: the caller flags the line for the host to render.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PGA_HD __host__ __device__ __forceinline__
#else
#define PGA_HD inline
#endif

namespace pga_fmt {

// Appends characters at p[n] (or only counts them when p is null): the renderer's length pass and its write pass run the
// same code, so the two can never disagree on a line's length.
struct Sink {
    char* p;
    int64_t n;
    PGA_HD void put(const char c) { if (p) p[n] = c; n++; }
    PGA_HD void puts(const char* s) { while (*s) put(*s++); }
    PGA_HD void put_n(const char* s, const int64_t len) { for (int64_t i = 0; i < len; i++) put(s[i]); }
};

PGA_HD void put_u64(Sink& o, uint64_t v) {
    char d[20];
    int k = 0;
    do { d[k++] = (char)('0' + (int)(v % 10)); v /= 10; } while (v);
    while (k) o.put(d[--k]);
}

PGA_HD void put_i64(Sink& o, const int64_t v) {
    if (v < 0) { o.put('-'); put_u64(o, (uint64_t)0 - (uint64_t)v); }
    else put_u64(o, (uint64_t)v);
}

PGA_HD uint64_t pow10_u(const int nd) { return nd == 1 ? 10u : nd == 2 ? 100u : 1000u; }

// '%.{nd}f' % x for nd in {1, 2, 3}; false when x is outside what the exact path covers (see above)
PGA_HD bool fmt_fixed(Sink& o, const double x, const int nd) {
    union { double d; uint64_t u; } b;
    b.d = x;
    const bool neg = (b.u >> 63) != 0;
    const int bexp = (int)((b.u >> 52) & 0x7ff);
    const uint64_t frac = b.u & ((1ull << 52) - 1);
    const uint64_t p10 = pow10_u(nd);
    if (neg) o.put('-');
    // x = m * 2^e exactly
    uint64_t m;
    int e;
    if (bexp == 0) { m = frac; e = -1074; }
    else { m = frac | (1ull << 52); e = bexp - 1075; }
    if (bexp == 0x7ff || bexp >= 1075 + 1) {   // non-finite, or |x| >= 2^53
        o.put('0'); o.put('.');
        for (int i = 0; i < nd; i++) o.put('0');
        return false;
    }
    uint64_t q;                              // round(x * 10^nd), half to even
    if (e >= 0) {
        q = (m << e) * p10;                  // m << e < 2^53 here
    } else {
        const uint64_t v = m * p10;          // < 2^53 * 1000 < 2^63
        const int s = -e;
        if (s >= 64) {
            q = 0;                           // v < 2^63 <= the half unit: rounds down
        } else {
            q = v >> s;
            const uint64_t r = v & ((1ull << s) - 1), half = 1ull << (s - 1);
            if (r > half || (r == half && (q & 1))) q++;
        }
    }
    put_u64(o, q / p10);
    o.put('.');
    uint64_t f = q % p10;
    char d[3];
    for (int i = nd - 1; i >= 0; i--) { d[i] = (char)('0' + (int)(f % 10)); f /= 10; }
    for (int i = 0; i < nd; i++) o.put(d[i]);
    return true;
}

// true when x lies within `margin` of a rounding midpoint of '%.{nd}f': a value computed with a transcendental function (the
// confidence's exp) that may differ from the host's by an ulp could print differently there
PGA_HD bool near_midpoint(const double x, const int nd, const double margin) {
    const double p = (double)pow10_u(nd);
    const double t = (x < 0 ? -x : x) * p;
    if (!(t < 9.0e18)) return true;           // NaN, infinities and huge values: the host renders them
    const double fl = (double)(int64_t)t;     // t >= 0 and < 2^63 whenever the exact path applies
    const double d = t - fl - 0.5;
    return (d < 0 ? -d : d) < margin * p;
}

// ---- closed forms of the renderer's lengths and offsets (render.hip), here so that the host-side shim reaches them ----

// letters of a FASTA record body: the bases begin .. end of a gene FASTA record; the residues of a protein, one per whole codon,
// without the stop codon's unless the gene runs off the sequence at its stop (partial flags are in sequence orientation) or the
// stop is asked for
PGA_HD int64_t body_letters(const int64_t begin, const int64_t end, const int strand, const int partial_begin, const int partial_end,
                            const int protein, const int include_stop) {
    const int64_t n = end - begin + 1;
    if (!protein) return n;
    const bool stop_edge = strand == 1 ? partial_end != 0 : partial_begin != 0;
    const int64_t l = n / 3 - ((!stop_edge && !include_stop) ? 1 : 0);
    return l > 0 ? l : 0;
}

constexpr int64_t kOriginLong = 16666667;   // first ORIGIN line whose position 60 k + 1 has ten digits ('{:>9}' widens)

// ORIGIN of a sequence of n bases: "ORIGIN\n", per 60 bases the position right-aligned in 9 columns and ten-base blocks with a
// leading space each, then "//\n"
PGA_HD int64_t origin_len(const int64_t n) {
    const int64_t lines = (n + 59) / 60;
    return 7 + 9 * lines + (lines > kOriginLong ? lines - kOriginLong : 0) + n + (n + 9) / 10 + lines + 3;
}
// first byte of ORIGIN line k (every line before it is full)
PGA_HD int64_t origin_line_at(const int64_t k) { return 7 + 76 * k + (k > kOriginLong ? k - kOriginLong : 0); }

// bytes of a '/translation="..."' string of L characters wrapped into 59-character pieces, every piece on a qualifier line:
// 21 spaces + piece + newline
PGA_HD int64_t gbk_tr_bytes(const int64_t L) { return L + 22 * ((L + 58) / 59); }

}  // namespace pga_fmt
