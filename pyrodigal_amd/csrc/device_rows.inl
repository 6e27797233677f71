// The host side that the calls which write device tensors share, and the rows some of them write.  DevCall: the
// refusals, the shared checks of records, tables and destinations, and the tail of a call -- for all of pga_translate_genes_tokens,
// pga_label_bases, pga_gene_windows, pga_count_kmers, pga_group_proteins, pga_sketch_proteins, pga_sketch_pairs, pga_cluster_sketches,
// pga_align_pairs, pga_cluster_edges and the pga_start_plan_* calls.  Staging: the tables of a call laid out in the upload lease.  RowDest, on top of DevCall: rows of 1-, 4- or
// 8-byte elements in a caller's tensor, ragged or padded, at any element alignment, which k_translate_tokens (translate_tokens.inl),
// k_label_bases (label_bases.inl) and k_gene_windows (gene_windows.inl) write.  Included by translate.hip, inside its anonymous
// namespace, in front of the kernel files.

constexpr int kRowThreads = 256;

template <int EB> struct TokElem;
template <> struct TokElem<1> { using type = uint8_t; };
template <> struct TokElem<4> { using type = int32_t; };
template <> struct TokElem<8> { using type = int64_t; };

// what a kernel is told about the destination, by value.  Element e of the layout lies at out0 + (lead + e) * elem_bytes: out0 is the
// 16-byte aligned address at or below d_out, lead the elements between the two (0 .. 16 / elem_bytes - 1)
struct RowArgs {
    const int64_t* off;        // [n_rows + 1] exclusive scan of len_g (both layouts: len_g = off[g + 1] - off[g])
    int64_t n_rows;
    int64_t n_elems;           // elements of the layout: off[n_rows], or (n_rows - 1) S + W
    int64_t W, S;              // padded layout
    int64_t pad;
    int32_t lead, _pad;
    char* out0;
};

// ---- the host side of a call that writes such rows ----

// <EB, PADDED> as types for a generic lambda: f(std::integral_constant<int, EB>, std::bool_constant<PADDED>)
template <typename F>
void with_elem_layout(const int eb, const bool padded, F f) {
    auto layout = [&](auto EB) { if (padded) f(EB, std::true_type{}); else f(EB, std::false_type{}); };
    if (eb == 1) layout(std::integral_constant<int, 1>{});
    else if (eb == 4) layout(std::integral_constant<int, 4>{});
    else layout(std::integral_constant<int, 8>{});
}

// A call on the context: its refusals, and the steps that every call which writes device tensors takes.  Each check returns PGA_OK
// or the refusal, its message in c->err; an entry point calls them in the order in which it refuses.
struct DevCall {
    pga_ctx* c; const char* fn;

    int bad(const std::string& msg) { c->err = std::string(fn) + ": " + msg; return PGA_EINVAL; }

    int contig_known(const pga_batch_view& bv, const pga_gene& G, const int64_t g) {
        if (G.contig < 0 || G.contig >= bv.n) return bad("gene " + std::to_string(g) + " names contig " + std::to_string(G.contig) + " of " + std::to_string(bv.n));
        return PGA_OK;
    }
    // record g inside its contig (gene_inside: the rule of the calls that read proteins)
    int record_inside(const pga_batch_view& bv, const pga_gene& G, const int64_t g) {
        return gene_inside(bv, G) ? PGA_OK : bad("gene " + std::to_string(g) + " lies outside its contig");
    }
    // record g inside its contig, in whole codons, across the origin only on a contig flagged circular: the rule of the calls that read
    // bases, with a message for each way to miss it
    int whole_codon_record(const pga_batch_view& bv, const pga_gene& G, const int64_t g) {
        if (const int rc = contig_known(bv, G, g)) return rc;
        const int64_t len = bv.ct[G.contig].len, glen = (int64_t)G.end - G.begin + 1;
        if (G.begin < 1 || G.begin > len || glen < 3 || glen > len) return bad("gene " + std::to_string(g) + " lies outside its contig");
        if (glen % 3) return bad("gene " + std::to_string(g) + " is " + std::to_string(glen) + " bases long, no whole number of codons");
        if (G.end > len && !(bv.circular && bv.circular[G.contig])) return bad("gene " + std::to_string(g) + " ends beyond its contig, which is not flagged circular");
        return PGA_OK;
    }
    int tables_known(const pga_batch_view& bv, const int32_t* table_of_contig) {
        for (int i = 0; i < bv.n; i++)
            if (!table_known(table_of_contig[i])) return bad("contig " + std::to_string(i) + ": " + std::to_string(table_of_contig[i]) + " is not a valid translation table index");
        return PGA_OK;
    }

    // The device pointers of a call.  kRequired: refused when NULL; kOptional: NULL leaves it out; kUnread: the call will not read it,
    // only its alignment is looked at.  First every NULL, then every alignment (`in_turn`: both, pointer after pointer), then every
    // pointer that is read must be device memory of the context's device.
    enum Need { kUnread = -1, kOptional = 0, kRequired = 1 };
    struct Dest { const char* name; const void* p; int elem_bytes; int need; };
    int destinations(std::initializer_list<Dest> ds, const bool in_turn = false) {
        auto missing = [](const Dest& x) { return x.need == kRequired && !x.p; };
        if (!in_turn) for (const Dest& x : ds) if (missing(x)) return bad(std::string(x.name) + " is NULL");
        for (const Dest& x : ds) {
            if (in_turn && missing(x)) return bad(std::string(x.name) + " is NULL");
            if ((uintptr_t)x.p % (uintptr_t)x.elem_bytes) return bad(std::string(x.name) + " is not aligned to its " + std::to_string(x.elem_bytes) + "-byte elements");
        }
        if (hipSetDevice(c->device) != hipSuccess) return PGA_EDEVICE;
        for (const Dest& x : ds) if (x.p && x.need != kUnread) if (const int rc = pga_device_memory_(c, x.p, fn, x.name)) return rc;
        return PGA_OK;
    }

    // The tail of a call: the first `bytes` of the lease's pinned area go up behind what the caller's stream held when the call came
    // (the upload stream is non-blocking), work(L.st) enqueues there and returns what HIP said (it may wait for the stream itself), and
    // on return the tensors are complete for any stream.  landed() runs once all of it is done and went well: what came back into the
    // pinned area is read there.  The stream is idle when the lease goes back, also after a failure: nothing of it is still in use.
    template <typename Work, typename Landed>
    int run(const pga_upload_lease& L, const size_t bytes, void* stream, Work work, Landed landed) {
        hipError_t e = hipEventRecord(L.ev, (hipStream_t)stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(L.st, L.ev, 0);
        if (e == hipSuccess && bytes > 0) e = hipMemcpyAsync(L.dev, L.pin, bytes, hipMemcpyHostToDevice, L.st);
        if (e == hipSuccess) e = work(L.st);
        const hipError_t es = hipStreamSynchronize(L.st);
        if (e == hipSuccess) e = es;
        if (e == hipSuccess) landed();
        pga_upload_lease_give(c);
        return pga_hip_try_(c, e, fn);
    }
    template <typename Work>
    int run(const pga_upload_lease& L, const size_t bytes, void* stream, Work work) { return run(L, bytes, stream, work, [] {}); }
};

// The tables of a call as they will lie in the upload lease: consecutive slices, each begun at a multiple of `align`.  The slices are
// named first -- put: bytes to copy there, take: room only -- and return their offset; lease() takes bytes() of the context's lease
// and copies what was put into its pinned area; then pin<T>(offset) / dev<T>(offset) are the two addresses of a slice.
struct Staging {
    const size_t align;
    pga_upload_lease L{};
    explicit Staging(const size_t align_ = 1) : align(align_) {}
    size_t take(const size_t bytes) { const size_t at = end_; end_ = (at + bytes + align - 1) / align * align; return at; }
    size_t put(const void* src, const size_t bytes) { src_.push_back({take(bytes), src, bytes}); return src_.back().at; }
    size_t bytes() const { return end_; }
    int lease(pga_ctx* c) {
        if (const int rc = pga_upload_lease_take(c, end_, &L)) return rc;
        for (const Src& s : src_) if (s.n) memcpy(L.pin + s.at, s.p, s.n);
        return PGA_OK;
    }
    template <typename T> T* pin(const size_t at) const { return (T*)(L.pin + at); }
    template <typename T> T* dev(const size_t at) const { return (T*)(L.dev + at); }
private:
    struct Src { size_t at; const void* p; size_t n; };
    size_t end_ = 0;
    std::vector<Src> src_;
};

// The caller's destination of a call that writes rows, and the RowArgs that describe it.
struct RowDest : DevCall {
    int eb = 0; bool padded = false;
    RowArgs a{};

    RowDest(pga_ctx* ctx, const char* name) : DevCall{ctx, name} {}
    const char* elem_name() const { return eb == 1 ? "uint8" : eb == 4 ? "int32" : "int64"; }
    int format(const int elem_bytes, const int layout) {
        eb = elem_bytes;
        if (eb != 1 && eb != 4 && eb != 8) return bad("elem_bytes must be 1, 4 or 8, not " + std::to_string(eb));
        if (layout != PGA_TOKENS_RAGGED && layout != PGA_TOKENS_PADDED) return bad("layout must be PGA_TOKENS_RAGGED or PGA_TOKENS_PADDED, not " + std::to_string(layout));
        padded = layout == PGA_TOKENS_PADDED;
        return PGA_OK;
    }
    // an id that goes into the tensor fits its elements (`what`: "vocab[65]", "pad", ...)
    bool fit(const int64_t v) const { return eb == 8 || (eb == 4 ? v >= INT32_MIN && v <= INT32_MAX : v >= 0 && v <= 255); }
    int fits(const std::string& what, const int64_t v) {
        return fit(v) ? PGA_OK : bad(what + " = " + std::to_string(v) + " does not fit " + elem_name());
    }
    int fits(const char* table, const int64_t* v, const int n) {
        for (int k = 0; k < n; k++) if (!fit(v[k])) return fits(std::string(table) + "[" + std::to_string(k) + "]", v[k]);
        return PGA_OK;
    }
    // the elements of the layout against what the caller gave
    int room(const int64_t n_out_elems) {
        if (n_out_elems < a.n_elems) return bad("n_out_elems = " + std::to_string(n_out_elems) + " is less than the " + std::to_string(a.n_elems) + " elements of the layout");
        return PGA_OK;
    }
    // the layout against the rows' lengths (`off`: their exclusive scan), `units of row` naming the longest ("tokens of gene")
    int shape(const std::vector<int64_t>& off, const char* units_of_row, const int64_t W, const int64_t S, const int64_t pad, const int64_t n_out_elems) {
        const int64_t n = (int64_t)off.size() - 1;
        int64_t longest = 0, longest_g = -1;
        for (int64_t g = 0; g < n; g++) if (off[g + 1] - off[g] > longest) { longest = off[g + 1] - off[g]; longest_g = g; }
        a.n_rows = n; a.n_elems = off[n];
        if (padded) {
            if (W < longest) return bad("row_width = " + std::to_string(W) + " is less than the " + std::to_string(longest) + " " + units_of_row + " " + std::to_string(longest_g));
            if (W < 0 || S < W) return bad("row_stride = " + std::to_string(S) + " is less than row_width = " + std::to_string(W));
            if (n > 1 && S > (INT64_MAX / 8 - W) / (n - 1)) return bad("row_stride = " + std::to_string(S) + " is too large");
            a.n_elems = n > 0 ? (n - 1) * S + W : 0;
            a.W = W; a.S = S; a.pad = pad;
        }
        return room(n_out_elems);
    }
    int memory(void* d_out) {
        if (a.n_elems == 0) return PGA_OK;
        if (const int rc = destinations({{"d_out", d_out, eb, kRequired}})) return rc;
        a.out0 = (char*)((uintptr_t)d_out & ~(uintptr_t)15);
        a.lead = (int32_t)(((uintptr_t)d_out - (uintptr_t)a.out0) / (uintptr_t)eb);
        return PGA_OK;
    }
    // the tail (DevCall::run) with launch(grid, block, stream): a thread per 16 bytes of the layout
    template <typename Launch>
    int run(const Staging& s, void* stream, Launch launch) {
        const int64_t per = 16 / eb, pieces = (a.lead + a.n_elems + per - 1) / per;
        return DevCall::run(s.L, s.bytes(), stream, [&](hipStream_t st) {
            launch(dim3((unsigned)((pieces + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), st);
            return hipGetLastError();
        });
    }
};
