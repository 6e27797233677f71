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

}
