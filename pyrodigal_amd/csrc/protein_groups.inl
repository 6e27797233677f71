// Gene records with the same predicted protein, or the same nucleotides, grouped on the device, exactly (pga_group_proteins; the rule
// is in pyrodigal_amd.h).  Included by translate.hip, inside its anonymous namespace, behind device_rows.inl: the
// __constant__ code tables and translate_rules.h are shared with k_translate.  A digest of every record's string, a stable radix sort
// of (digest word 0, record index), and a comparison of the strings themselves inside every run of equal keys: a hash only says which
// pairs are worth comparing.  Of the batch, only the records' own letters are read.

// One record, built on the host from a checked one: the 88-byte gene records do not go up.  Unit x of the string (a residue or a base)
// begins at 0-based position q0 + step x on a forward record and q0 - step x on a reverse one, step = 3 or 1; a position p >= L (a
// record across the origin of a circle) reads p - L.  On either strand 0 <= p < 2 L.
struct GrpRow {
    int64_t base;              // the contig's first letter in the batch
    int32_t q0;
    int32_t L;
    int32_t n;                 // units of the string: residues or bases
    uint32_t bits;             // bit 0: forward.  Bit 1: the record's own first codon lies at an edge.  Bits 8 ..: the translation table
};
static_assert(sizeof(GrpRow) == 24, "GrpRow");

constexpr int kGrpProtein = 0, kGrpGene = 1;
constexpr uint64_t kGrpM = (1ull << 61) - 1, kGrpB0 = 0x0123456789ABCDEFull, kGrpB1 = 0x1BADB002C0FFEE11ull;
constexpr int kGrpLanes = 16;                                  // lanes that share one record in k_string_digest: four records per wave

// everything the kernels are told, by value
struct GrpArgs {
    const char* seq; const GrpRow* row;
    int64_t n;                                                 // G
    int32_t unk, strict;
    int32_t precheck, _pad;                                    // 0 under PGA_PROTEIN_GROUPS_KEY_BITS: the strings alone decide
    uint64_t key_mask;                                         // the bits of word 0 the sort looked at
    uint64_t* w0; uint64_t* w1;                                // [G] the digest
    uint32_t* idx;                                             // [G] 0 .. G - 1: the sort's values
    const uint64_t* skey; const uint32_t* sidx;                // [G] sorted
    uint32_t* start; uint32_t* runstart;                       // [G] i at the first position of a run, else 0; its running maximum
    uint32_t* cand; uint32_t* cand_next;                       // [G] at a run's first position: the position of its head in this round / the next
    int32_t* head;                                             // [G] by record: the representative, -1 while unresolved
    unsigned long long* unresolved;                            // the members a round left for the next
    int64_t* d_digest;                                         // [G, 2] or nullptr
};

// a b mod 2^61 - 1 for a, b < 2^61: the 122-bit product folded twice
__device__ __forceinline__ uint64_t grp_mul(const uint64_t a, const uint64_t b) {
    const uint64_t lo = a * b, hi = __umul64hi(a, b);
    uint64_t s = (lo & kGrpM) + ((hi << 3) | (lo >> 61));      // < 2^62
    s = (s & kGrpM) + (s >> 61);
    return s >= kGrpM ? s - kGrpM : s;
}
__device__ __forceinline__ uint64_t grp_add(const uint64_t a, const uint64_t b) {      // a, b < M
    const uint64_t s = a + b;
    return s >= kGrpM ? s - kGrpM : s;
}
__device__ __forceinline__ uint64_t grp_pow(uint64_t b, uint32_t e) {
    uint64_t r = 1;
    for (; e; e >>= 1) { if (e & 1u) r = grp_mul(r, b); b = grp_mul(b, b); }
    return r;
}

// unit x of a record's string: the residue of codon x as tok_at reads it, or base x as k_gene_windows reads it
template <int UNIT>
__device__ __forceinline__ int grp_unit(const GrpArgs& a, const GrpRow& w, const int x) {
    const char* __restrict__ s = a.seq + w.base;
    const bool fwd = (w.bits & 1u) != 0u;
    auto at = [&](const int p) { return s[p >= w.L ? p - w.L : p]; };
    if (UNIT == kGrpGene) {
        int c;
        switch (at(fwd ? w.q0 + x : w.q0 - x)) { case 'A': case 'a': c = 0; break; case 'C': case 'c': c = 1; break; case 'G': case 'g': c = 2; break;
                                                  case 'T': case 't': c = 3; break; default: return 'N'; }
        if (!fwd) c = 3 - c;                                   // A <-> T, C <-> G
        return c == 0 ? 'A' : c == 1 ? 'C' : c == 2 ? 'G' : 'T';
    }
    const int tt = (int)(w.bits >> 8);
    int x0, x1, x2;
    if (fwd) {
        const int p = w.q0 + 3 * x;
        x0 = digit_of(at(p), false); x1 = digit_of(at(p + 1), false); x2 = digit_of(at(p + 2), false);
    } else {
        const int p = w.q0 - 3 * x;
        x0 = digit_of(at(p), true); x1 = digit_of(at(p - 1), true); x2 = digit_of(at(p - 2), true);
    }
    return translate_codon(c_code[tt], x0, x1, x2, tt, x, (w.bits & 2u) != 0u, a.strict, a.unk) & 0xff;
}

// The digest of every record.  Work is dealt by wave, and a wave takes four records at a time in a loop, kGrpLanes lanes each: a lane
// runs Horner over a contiguous share of the record's units under both bases and carries (hash of the share, b ^ its length); the lanes
// of a record combine their pairs in lane order with the associative (h1, p1) o (h2, p2) = (h1 p2 + h2, p1 p2) -- a lane without
// units holds the identity (0, 1) -- and the first lane adds b ^ n for the leading 1.  One 10 000-residue record and 200 000 short ones
// both go through this.
template <int UNIT>
__global__ void __launch_bounds__(kRowThreads)
k_string_digest(const GrpArgs a) {
    const int sub = threadIdx.x & (kGrpLanes - 1);
    const int64_t per = kRowThreads / kGrpLanes;
    for (int64_t g = (int64_t)blockIdx.x * per + threadIdx.x / kGrpLanes; g < ((a.n + 3) & ~(int64_t)3); g += (int64_t)gridDim.x * per) {
        // (the four records of a wave leave the loop together: the shuffles below see whole groups)
        const bool live = g < a.n;
        GrpRow w{};
        if (live) w = a.row[g];
        const int share = (w.n + kGrpLanes - 1) / kGrpLanes;
        const int lo = min(sub * share, w.n), hi = min(lo + share, w.n);
        uint64_t h0 = 0, h1 = 0;
        for (int x = lo; x < hi; x++) {
            const uint64_t r = (uint64_t)grp_unit<UNIT>(a, w, x);
            h0 = grp_add(grp_mul(h0, kGrpB0), r);
            h1 = grp_add(grp_mul(h1, kGrpB1), r);
        }
        uint64_t p0 = grp_pow(kGrpB0, (uint32_t)(hi - lo)), p1 = grp_pow(kGrpB1, (uint32_t)(hi - lo));
#pragma unroll
        for (int d = 1; d < kGrpLanes; d <<= 1) {
            const uint64_t rh0 = __shfl_down(h0, d, kGrpLanes), rp0 = __shfl_down(p0, d, kGrpLanes);
            const uint64_t rh1 = __shfl_down(h1, d, kGrpLanes), rp1 = __shfl_down(p1, d, kGrpLanes);
            if (sub + d < kGrpLanes) {                         // (beyond the group's last lane: the identity)
                h0 = grp_add(grp_mul(h0, rp0), rh0); p0 = grp_mul(p0, rp0);
                h1 = grp_add(grp_mul(h1, rp1), rh1); p1 = grp_mul(p1, rp1);
            }
        }
        if (live && sub == 0) {
            const uint64_t v0 = grp_add(p0, h0), v1 = grp_add(p1, h1);
            a.w0[g] = v0; a.w1[g] = v1; a.idx[g] = (uint32_t)g;
            if (a.d_digest) { a.d_digest[2 * g] = (int64_t)v0; a.d_digest[2 * g + 1] = (int64_t)v1; }
        }
    }
}

// the runs of equal keys in the sorted order: every run's first position, which is its head of round 0
__global__ void __launch_bounds__(kRowThreads)
k_group_runs(const GrpArgs a) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.n) return;
    const bool first = i == 0 || ((a.skey[i] ^ a.skey[i - 1]) & a.key_mask) != 0;
    a.start[i] = first ? (uint32_t)i : 0u;
    if (first) a.cand[i] = (uint32_t)i;
}

struct GrpMax { __host__ __device__ __forceinline__ uint32_t operator()(const uint32_t x, const uint32_t y) const { return x > y ? x : y; } };

// One round.  A lane looks at one sorted position: a record that is not yet resolved is its run's head -- the first unresolved member,
// which resolves to itself -- or is compared with the head: the length and digest word 1 first, by the lane, then the strings
// themselves by the whole wave, pair after pair, the lanes striding over the units with a vote that ends a pair at its first
// difference.  Equal: the member takes the head's record index.  Not equal: it stays for the next round, names itself for its run's
// next head (the smallest position wins: the run is in index order, the sort being stable) and is counted.
template <int UNIT>
__global__ void __launch_bounds__(kRowThreads)
k_group_verify(const GrpArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;          // (whole waves: the votes below see every lane)
    int g = -1, h = -1;
    uint32_t rs = 0;
    bool differs = false, compare = false;
    if (i < a.n) {
        g = (int)a.sidx[i];
        if (a.head[g] < 0) {
            rs = a.runstart[i];
            const uint32_t hp = a.cand[rs];
            if (hp == (uint32_t)i) a.head[g] = g;
            else {
                h = (int)a.sidx[hp];
                if (a.precheck && (a.row[g].n != a.row[h].n || a.w1[g] != a.w1[h])) differs = true; else compare = true;
            }
        }
    }
    unsigned long long todo = __ballot(compare);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const GrpRow wg = a.row[__shfl(g, src)], wh = a.row[__shfl(h, src)];
        bool ne = wg.n != wh.n;
        for (int x = lane; !ne && x - lane < wg.n; x += 64) {                 // (x - lane is the wave's: every lane leaves together)
            const bool d = x < wg.n && grp_unit<UNIT>(a, wg, x) != grp_unit<UNIT>(a, wh, x);
            if (__any(d)) ne = true;
        }
        if (lane == src) { if (ne) differs = true; else a.head[g] = h; }
    }
    if (differs) {
        atomicMin(&a.cand_next[rs], (uint32_t)i);
        atomicAdd(a.unresolved, 1ull);
    }
}

// ---- numbering: all integer, so the result depends on the arguments alone ----
struct GrpOut {
    const int32_t* head; int32_t* flag; const int32_t* num; int32_t* cnt; int64_t n;
    int64_t* d_group; int64_t* d_rep; int64_t* d_size; long long* n_groups;
};
__global__ void __launch_bounds__(kRowThreads)
k_group_flags(const GrpOut o) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= o.n) return;
    o.flag[g] = o.head[g] == (int32_t)g ? 1 : 0;
    o.cnt[g] = 0;
}
__global__ void __launch_bounds__(kRowThreads)
k_group_count(const GrpOut o) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= o.n) return;
    const int32_t h = o.head[g];
    o.d_group[g] = o.num[h];
    if (o.d_size) atomicAdd(&o.cnt[h], 1);
    if (g == o.n - 1) *o.n_groups = (long long)o.num[g] + o.flag[g];
}
__global__ void __launch_bounds__(kRowThreads)
k_group_emit(const GrpOut o) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= o.n || !o.flag[g]) return;
    if (o.d_rep) o.d_rep[o.num[g]] = g;
    if (o.d_size) o.d_size[o.num[g]] = o.cnt[g];
}
