// Rows of 1-, 4- or 8-byte elements written into a caller's device tensor, ragged or padded, at any element alignment (DESIGN.md
// 4.14): the destination's description and the host side of such a call, which k_translate_tokens (translate_tokens.inl),
// k_label_bases (label_bases.inl) and k_gene_windows (gene_windows.inl) share.  Included by translate.hip, inside its anonymous
// namespace, in front of the three.

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

// The caller's destination, checked on the host before anything is allocated or launched, and the RowArgs that describe it.  The
// steps are called in the order in which an entry point refuses: each returns PGA_OK or the refusal, its message in c->err.
struct RowDest {
    pga_ctx* c; const char* fn;
    int eb = 0; bool padded = false;
    RowArgs a{};

    int bad(const std::string& msg) { c->err = std::string(fn) + ": " + msg; return PGA_EINVAL; }
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
        if (n_out_elems < a.n_elems) return bad("n_out_elems = " + std::to_string(n_out_elems) + " is less than the " + std::to_string(a.n_elems) + " elements of the layout");
        return PGA_OK;
    }
    int memory(void* d_out) {
        if (a.n_elems == 0) return PGA_OK;
        if (!d_out) return bad("d_out is NULL");
        if ((uintptr_t)d_out % (uintptr_t)eb) return bad("d_out is not aligned to its " + std::to_string(eb) + "-byte elements");
        if (hipSetDevice(c->device) != hipSuccess) return PGA_EDEVICE;
        if (const int rc = pga_device_memory_(c, d_out, fn, "d_out")) return rc;
        a.out0 = (char*)((uintptr_t)d_out & ~(uintptr_t)15);
        a.lead = (int32_t)(((uintptr_t)d_out - (uintptr_t)a.out0) / (uintptr_t)eb);
        return PGA_OK;
    }
    // The tail of the call: the `tab` bytes staged in the lease go up behind what the caller's stream held when the call came (the
    // upload stream is non-blocking), launch(grid, block, stream) runs there, and on return the tensor is complete for any stream.
    template <typename Launch>
    int run(pga_upload_lease& L, const size_t tab, void* stream, Launch launch) {
        const int64_t per = 16 / eb, pieces = (a.lead + a.n_elems + per - 1) / per;
        hipError_t e = hipEventRecord(L.ev, (hipStream_t)stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(L.st, L.ev, 0);
        if (e == hipSuccess) e = hipMemcpyAsync(L.dev, L.pin, tab, hipMemcpyHostToDevice, L.st);
        if (e == hipSuccess) {
            launch(dim3((unsigned)((pieces + kRowThreads - 1) / kRowThreads)), dim3(kRowThreads), L.st);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipStreamSynchronize(L.st);
        pga_upload_lease_give(c);
        return pga_hip_try_(c, e, fn);
    }
};
