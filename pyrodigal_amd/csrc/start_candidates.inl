// Every candidate start site of a gene record's ORF with its scores, left on the device as three tensors (pga_start_plan_create /
// pga_start_plan_write; the rule is in pyrodigal_amd.h).  Included by translate.hip, inside its anonymous namespace,
// behind device_rows.inl.  Both kernels read the kept node arena in stopcmp_nodes order (pga_node_order, render.hip): the starts of
// one ORF are the rows of one key there, in ndx order.

// what the host sends of a checked record: the 88-byte gene records do not go up
struct StartReq { int32_t contig, x /* arena index of its start node */, pos /* begin (forward) or end (reverse) */, strand; };
static_assert(sizeof(StartReq) == 16, "StartReq");
// why the look-up kernel refuses a record: the count it reports is minus one of these
constexpr int kStartIsStop = 1, kStartStrand = 2, kStartPosition = 3, kStartLost = 4;

// The group of every record, a thread per record: the rows of its key (contig, stop_val, strand) by binary search in the sorted keys,
// inside the contig's rows; then the record's own row by a second search on the arena index inside the group (the sort is stable and
// the arena is in ndx order, so the indices of a group ascend).  Rank is counted from the far end on the reverse strand.
// grp[g] = (first sorted row, n_g, negative on the reverse strand); res[g] = (n_g or minus a refusal, chosen_g): what goes home.
__global__ void __launch_bounds__(kRowThreads)
k_start_lookup(const DevNodeArrays nd, const uint64_t* __restrict__ skey, const uint32_t* __restrict__ sval, const int64_t* __restrict__ srow,
               const int n_contigs, const StartReq* __restrict__ req, const int64_t n_genes, int2* __restrict__ grp, int2* __restrict__ res) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_genes) return;
    const StartReq q = req[g];
    const int64_t x = q.x;
    const int type = nd.type[x], strand = nd.strand[x];
    int bad = 0;
    if (type == PGA_T_STOP) bad = kStartIsStop;
    else if (strand != q.strand) bad = kStartStrand;
    else if (nd.ndx[x] + 1 != q.pos) bad = kStartPosition;
    int64_t lo = 0, hi = 0, r = 0;
    if (!bad) {
        const uint64_t key = pga_node_order_key(n_contigs, q.contig, type, nd.stop_val[x], strand);
        const int64_t r0 = srow[q.contig], r1 = srow[q.contig + 1];
        int64_t l = r0, h = r1;                                      // first row with skey >= key
        while (l < h) { const int64_t mid = (l + h) >> 1; if (skey[mid] < key) l = mid + 1; else h = mid; }
        lo = l; h = r1;                                              // first row with skey > key
        while (l < h) { const int64_t mid = (l + h) >> 1; if (skey[mid] <= key) l = mid + 1; else h = mid; }
        hi = l;
        l = lo; h = hi;                                              // first row of the group with sval >= x
        while (l < h) { const int64_t mid = (l + h) >> 1; if ((int64_t)sval[mid] < x) l = mid + 1; else h = mid; }
        r = l;
        if (r >= hi || (int64_t)sval[r] != x) bad = kStartLost;       // (the arena and the order disagree: never with a node of the contig)
    }
    if (bad) { grp[g] = make_int2(0, 0); res[g] = make_int2(-bad, 0); return; }
    const int n = (int)(hi - lo);
    const bool fwd = strand == 1;
    grp[g] = make_int2((int)lo, fwd ? n : -n);
    res[g] = make_int2(n, (int)(fwd ? r - lo : hi - 1 - r));
}

// the arena index of every candidate in ragged order (pga_start_plan_nodes): the write kernel's walk without the gather
__global__ void __launch_bounds__(kRowThreads)
k_start_nodes(const uint32_t* __restrict__ sval, const int2* __restrict__ grp, const int64_t* __restrict__ off, const int64_t n_genes,
              const int64_t n_cells, uint32_t* __restrict__ out) {
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= n_cells) return;
    int64_t l = 0, h = n_genes - 1;
    while (l < h) { const int64_t mid = (l + h + 1) >> 1; if (off[mid] <= cell) l = mid; else h = mid - 1; }
    const int2 gr = grp[l];
    const int64_t k = cell - off[l], n = gr.y < 0 ? -gr.y : gr.y;
    out[cell] = sval[(int64_t)gr.x + (gr.y < 0 ? n - 1 - k : k)];
}

template <int B> struct StartIndex;
template <> struct StartIndex<4> { using type = int32_t; };
template <> struct StartIndex<8> { using type = int64_t; };
template <int B> struct StartScore;
template <> struct StartScore<4> { using type = float; };
template <> struct StartScore<8> { using type = double; };

// everything the write kernel is told, by value
struct StartArgs {
    DevNodeArrays nd;
    const uint32_t* sval;      // the arena index of every sorted row
    const int2* grp;           // per record: first sorted row, n_g (negative: reverse strand)
    const int64_t* off;        // [n_genes + 1] exclusive scan of n_g
    int64_t n_genes;
    int64_t n_cells;           // candidates the launch runs over: T (ragged) or G W (padded)
    int64_t W, S;              // padded layout
    int64_t index_pad; double score_pad;
    int32_t n_fields; int32_t fields[7];
    void* pos; void* typ; void* sco;
};

// Work is dealt by candidates, not by genes: an ORF with 500 starts costs what 500 ORFs with one start cost.  A thread owns one cell --
// candidate k of row g, found by binary search in `off` (ragged) or from the cell index (padded), the pad cells of a padded row among
// them -- gathers its node's position and type from the arena and stores them, neighbours to neighbours.  The scores are [.., F] with F
// of 1 .. 7: the workgroup leaves every cell's arena index and destination in LDS and then walks its 256 F score elements in element
// order, so a wave's stores are as contiguous as the rows are, whatever F is.  The field codes sit in LDS beside them (the column
// diverges per lane).  Nothing but the elements the rule names is written.
template <int IB, int SB, bool PADDED>
__global__ void __launch_bounds__(kRowThreads)
k_start_candidates(const StartArgs a) {
    using I = typename StartIndex<IB>::type;
    using F = typename StartScore<SB>::type;
    __shared__ int64_t s_e[kRowThreads];       // the cell's element in positions / types; scores: s_e F + column
    __shared__ int32_t s_x[kRowThreads];       // its node in the arena, -1: a pad cell, -2: no cell
    __shared__ int32_t s_field[8];
    const int tid = threadIdx.x;
    {
        int f = 0;                             // (constant indices: a.fields stays in the kernel's arguments)
#pragma unroll
        for (int k = 0; k < 7; k++) if (tid == k) f = a.fields[k];
        if (tid < 7) s_field[tid] = f;
    }
    const DevNodeArrays& N = a.nd;
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + tid;
    int32_t x = -2;
    int64_t e = 0;
    if (cell < a.n_cells) {
        int64_t g, k;
        if (PADDED) {
            g = cell / a.W; k = cell - g * a.W; e = g * a.S + k;
        } else {
            // the last row that begins at or before the cell: it is not empty (n_g >= 1 for every row)
            int64_t l = 0, h = a.n_genes - 1;
            while (l < h) { const int64_t mid = (l + h + 1) >> 1; if (a.off[mid] <= cell) l = mid; else h = mid - 1; }
            g = l; k = cell - a.off[g]; e = cell;
        }
        const int2 gr = a.grp[g];
        const int n = gr.y < 0 ? -gr.y : gr.y;
        x = -1;
        if (k < n) x = (int32_t)a.sval[(int64_t)gr.x + (gr.y < 0 ? n - 1 - k : k)];
        I* __restrict__ const pos = reinterpret_cast<I*>(a.pos);
        I* __restrict__ const typ = reinterpret_cast<I*>(a.typ);
        pos[e] = x >= 0 ? (I)((int64_t)N.ndx[x] + 1) : (I)a.index_pad;
        typ[e] = x >= 0 ? (I)(N.edge[x] ? 3 : (N.type[x] & 3)) : (I)a.index_pad;
    }
    s_x[tid] = x; s_e[tid] = e;
    __syncthreads();
    F* __restrict__ const sco = reinterpret_cast<F*>(a.sco);
    const int nf = a.n_fields;
    for (int i = tid; i < kRowThreads * nf; i += kRowThreads) {
        const int cl = i / nf, f = i - cl * nf;
        const int32_t y = s_x[cl];
        if (y == -2) continue;
        double v = a.score_pad;
        if (y >= 0) {
            switch (s_field[f]) {
                case PGA_START_TOTAL:  v = N.cscore[y] + N.sscore[y]; break;
                case PGA_START_CSCORE: v = N.cscore[y]; break;
                case PGA_START_SSCORE: v = N.sscore[y]; break;
                case PGA_START_RSCORE: v = N.rscore[y]; break;
                case PGA_START_USCORE: v = N.uscore[y]; break;
                case PGA_START_TSCORE: v = N.tscore[y]; break;
                default:               v = (double)N.gc_cont[y]; break;
            }
        }
        sco[s_e[cl] * nf + f] = (F)v;
    }
}
