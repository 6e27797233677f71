// Host-only build of pyrodigal_amd/csrc/render_fmt.h for tests/test_render_format_cpu.py.
#include "../pyrodigal_amd/csrc/render_fmt.h"

extern "C" {

// '%.{nd}f' of every x[i], each followed by '\n'; returns the bytes written (out must hold 32 bytes per value).
// ok[i] = 0 where the exact path did not apply.
int64_t render_fmt_many(const double* x, int64_t n, int nd, char* out, unsigned char* ok) {
    pga_fmt::Sink o{out, 0};
    for (int64_t i = 0; i < n; i++) {
        ok[i] = pga_fmt::fmt_fixed(o, x[i], nd) ? 1 : 0;
        o.put('\n');
    }
    return o.n;
}

int render_near_midpoint(double x, int nd, double margin) { return pga_fmt::near_midpoint(x, nd, margin) ? 1 : 0; }

// put_i64 of v into out (24 bytes); returns the characters written
int64_t render_put_i64(int64_t v, char* out) {
    pga_fmt::Sink o{out, 0};
    pga_fmt::put_i64(o, v);
    return o.n;
}

// the closed forms of the renderer's lengths and offsets
int64_t render_origin_len(int64_t n) { return pga_fmt::origin_len(n); }
int64_t render_origin_line_at(int64_t k) { return pga_fmt::origin_line_at(k); }
int64_t render_gbk_tr_bytes(int64_t L) { return pga_fmt::gbk_tr_bytes(L); }
int64_t render_body_letters(int64_t begin, int64_t end, int strand, int partial_begin, int partial_end, int protein, int include_stop) {
    return pga_fmt::body_letters(begin, end, strand, partial_begin, partial_end, protein, include_stop);
}

}
