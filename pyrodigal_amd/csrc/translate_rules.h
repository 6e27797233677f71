// Translation rules shared by the device translation (translate.hip) and the device renderer (render.hip): the NCBI genetic
// codes, the start and stop codons of every table and the digit alphabet of this library (A0 G1 C2 T3).
// ref: _sequence.h:19-73 (stop / start codons per table), _translation.h:4-42 (the genetic codes; restated here from the NCBI
// tables in TCAG order and re-indexed by the digit alphabet).
#pragma once

#include <hip/hip_runtime.h>
#include <string.h>

#include <initializer_list>

namespace pga_tr {

// NCBI genetic codes, 64 codons in TCAG order (first base slowest)
struct Code { int tt; const char* aa; };
inline constexpr Code NCBI[] = {
    {1, "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"}, {2, "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSS**VVVVAAAADDEEGGGG"},
    {3, "FFLLSSSSYY**CCWWTTTTPPPPHHQQRRRRIIMMTTTTNNKKSSRRVVVVAAAADDEEGGGG"}, {4, "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"},
    {5, "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSSSSVVVVAAAADDEEGGGG"}, {6, "FFLLSSSSYYQQCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"},
    {9, "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNNKSSSSVVVVAAAADDEEGGGG"}, {10, "FFLLSSSSYY**CCCWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"},
    {11, "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"}, {12, "FFLLSSSSYY**CC*WLLLSPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"},
    {13, "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSSGGVVVVAAAADDEEGGGG"}, {14, "FFLLSSSSYYY*CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNNKSSSSVVVVAAAADDEEGGGG"},
    {15, "FFLLSSSSYY*QCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"}, {16, "FFLLSSSSYY*LCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"},
    {21, "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNNKSSSSVVVVAAAADDEEGGGG"}, {22, "FFLLSS*SYY*LCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"},
    {23, "FF*LSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"}, {24, "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSSKVVVVAAAADDEEGGGG"},
    {25, "FFLLSSSSYY**CCGWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"}, {26, "FFLLSSSSYY**CC*WLLLAPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"},
    {29, "FFLLSSSSYYYYCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"}, {30, "FFLLSSSSYYEECC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"},
    {32, "FFLLSSSSYY*WCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"}, {33, "FFLLSSSSYYY*CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSSKVVVVAAAADDEEGGGG"},
};
__device__ __forceinline__ bool tt_in(const int tt, const unsigned long long set) { return (set >> tt) & 1ull; }
#define TTS(...) tts_of({__VA_ARGS__})
__device__ __host__ constexpr unsigned long long tts_of(std::initializer_list<int> l) { unsigned long long m = 0; for (int t : l) m |= 1ull << t; return m; }

// ref: _sequence.h:19-43
__device__ __forceinline__ bool codon_stop(const int x0, const int x1, const int x2, const int tt) {
    if (x0 == 0 && tt == 2) return x1 == 1 && (x2 == 0 || x2 == 1);                                   // AGA / AGG
    if (x0 != 3) return false;
    if (x1 == 0 && x2 == 1) return tt_in(tt, TTS(1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14, 21, 23, 24, 25, 26, 33));     // TAG
    if (x1 == 1 && x2 == 0) return tt_in(tt, TTS(1, 6, 11, 12, 15, 16, 22, 23, 26, 29, 30, 32));                      // TGA
    if (x1 == 0 && x2 == 0) return tt_in(tt, TTS(1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 15, 16, 21, 22, 23, 24, 25, 26, 32));   // TAA
    if (tt == 22) return x1 == 2 && x2 == 0;                                                            // TCA
    if (tt == 23) return x1 == 3 && x2 == 0;                                                            // TTA
    return false;
}
// ref: _sequence.h:45-73
__device__ __forceinline__ bool codon_start(const int x0, const int x1, const int x2, const int tt) {
    if (x1 != 3 || x2 != 1) return false;
    if (x0 == 0) return true;
    if (tt_in(tt, TTS(6, 10, 14, 15, 16, 2))) return false;
    if (x0 == 1) return !(tt == 1 || tt == 3 || tt == 12 || tt == 2);
    if (x0 == 3) return !(tt < 4 || tt == 9 || (tt >= 21 && tt < 25));
    return false;
}
__device__ __forceinline__ int digit_of(const int ch, const bool comp) {
    int d;
    switch (ch) { case 'A': case 'a': d = 0; break; case 'G': case 'g': d = 1; break; case 'C': case 'c': d = 2; break;
                  case 'T': case 't': d = 3; break; default: return 6; }
    return comp ? 3 - d : d;            // A <-> T, G <-> C
}

// one codon of a gene: i = codon index in the gene, row = the table's 64 residues indexed by digits (code_table())
__device__ __forceinline__ char translate_codon(const char* __restrict__ row, const int x0, const int x1, const int x2, const int tt,
                                                const int i, const bool start_edge, const int strict, const int unk) {
    int aa;
    if (x0 <= 3 && x1 <= 3 && x2 <= 3) {
        if (codon_stop(x0, x1, x2, tt)) aa = '*';
        else if (i == 0 && !start_edge && codon_start(x0, x1, x2, tt)) aa = 'M';
        else aa = row[(x0 << 4) + (x1 << 2) + x2];
    } else {
        aa = 'X';
        if (!strict && x0 <= 3 && (x1 <= 3) != (x2 <= 3)) {
            // one unknown base in second or third position: unambiguous when all four completions agree
            aa = row[(x0 << 4) + ((x1 <= 3 ? x1 : 0) << 2) + (x2 <= 3 ? x2 : 0)];
            for (int y = 1; y < 4; y++)
                if (row[(x0 << 4) + ((x1 <= 3 ? x1 : y) << 2) + (x2 <= 3 ? x2 : y)] != aa) { aa = 'X'; break; }
        }
    }
    return (char)(aa == 'X' ? unk : aa);
}

// the genetic codes by digits: code[tt][a << 4 | b << 2 | c]; all-zero rows = unknown tables
inline void code_table(char code[34][64], unsigned char known[34]) {
    memset(code, 0, 34 * 64); memset(known, 0, 34);
    const int ncbi_of_digit[4] = {2, 3, 1, 0};        // digit (A G C T) -> position in TCAG
    for (const Code& c : NCBI) {
        known[c.tt] = 1;
        for (int a = 0; a < 4; a++) for (int b = 0; b < 4; b++) for (int d = 0; d < 4; d++)
            code[c.tt][(a << 4) + (b << 2) + d] = c.aa[ncbi_of_digit[a] * 16 + ncbi_of_digit[b] * 4 + ncbi_of_digit[d]];
    }
}
inline bool table_known(const int tt) { for (const Code& c : NCBI) if (c.tt == tt) return true; return false; }

}  // namespace pga_tr
