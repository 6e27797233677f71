// Host-only build of pyrodigal_amd/csrc/knobs.h for tests/test_knobs_cpu.py: the fields of a fresh read_knobs(), or of
// process_knobs(), as a flat array in the order of knobs_field_names().
// With -DKNOBS_MAIN the file is a stand-alone program that reads a handful of settings (for a sanitizer build).
#include "../pyrodigal_amd/csrc/knobs.h"

#include <stdio.h>

#define KNOB_FIELDS(F) \
    F(timing) F(fault_contig_len_set) F(fault_contig_len) F(pageable_results) F(cache_gb) F(upload_turns) F(mallopt) F(dp_seg_height) F(dpw_occ) \
    F(print_buffers) F(fasta_no_mmap) F(fasta_threads) F(stage_full) F(stage_shift_set) F(stage_shift) F(extract_c) F(extract_pool) F(cs_lds) \
    F(cs_task_nodes) F(cs_wave) F(cs_qclasses) F(cs_profile) F(ss_starts_only) F(ss_mm) F(ss_mm_tile) F(ss_models_per_pass) F(ss_full_stops) \
    F(ss_profile) F(ovl_search) F(dp_kernel_set) F(dp_kernel) F(dp_waves) F(dp_profile) F(dp_seg) F(dp_seg_min) F(dp_seg_warm) F(dp_seg_len_set) \
    F(dp_seg_len) F(dp_seg_slots) F(dp_seg_wslots) F(dp_seg_wave_set) F(dp_seg_wave) F(dp_seg_wave_min) F(dp_seg_readback) F(dp_seg_debug) \
    F(dp_no_order) F(dp_xcd) F(dpw_sched) F(dpw_sched_miss) F(dpw_sched_debug) F(dpw_topo_walk) F(dpw_topo_lds) F(tail) F(full_gather) \
    F(gather_all_dp) F(tp_steps) F(tp_jump8) F(tp_extract_one) F(tweak_slots) F(kmer_direct) F(kmer_per_wave) F(protein_groups_key_bits)

static int fill(const Knobs& k, int64_t* out) {
    int n = 0;
#define F(field) out[n++] = (int64_t)k.field;
    KNOB_FIELDS(F)
#undef F
    return n;
}

extern "C" {

// the field names, comma-separated, in the order knobs_read / knobs_process fill `out` (at most 128 entries)
const char* knobs_field_names() {
#define F(field) #field ","
    return KNOB_FIELDS(F);
#undef F
}
int knobs_read(int64_t* out) { return fill(read_knobs(), out); }                       // the environment as it is now
int knobs_process(int64_t* out) { return fill(pga_knobs::process_knobs(), out); }      // as it was when this was first called

}

#ifdef KNOBS_MAIN
static int64_t field(const char* name) {
    int64_t v[128];
    const int n = knobs_read(v);
    const char* p = knobs_field_names();
    for (int i = 0; i < n; i++) {
        const char* e = strchr(p, ',');
        if ((size_t)(e - p) == strlen(name) && !strncmp(p, name, e - p)) return v[i];
        p = e + 1;
    }
    return -12345;
}
static int bad = 0;
static void expect(const char* var, const char* value, const char* name, const int64_t want) {
    if (value) setenv(var, value, 1); else unsetenv(var);
    const int64_t got = field(name);
    if (got != want) { printf("%s=%s: %s is %lld, not %lld\n", var, value ? value : "(unset)", name, (long long)got, (long long)want); bad++; }
    unsetenv(var);
}
int main() {
    expect("PGA_CS_TASK_NODES", "255", "cs_task_nodes", 5120); expect("PGA_CS_TASK_NODES", "256", "cs_task_nodes", 256);
    expect("PGA_CS_TASK_NODES", "8192", "cs_task_nodes", 8192); expect("PGA_CS_TASK_NODES", "8193", "cs_task_nodes", 5120);
    expect("PGA_SS_MM_TILE", "300", "ss_mm_tile", 1024); expect("PGA_SS_MM_TILE", "512", "ss_mm_tile", 512);
    expect("PGA_EXTRACT_C", "-1", "extract_c", 0); expect("PGA_EXTRACT_C", "9", "extract_c", 4); expect("PGA_EXTRACT_C", "", "extract_c", 0);
    expect("PGA_STAGE_SHIFT", "99", "stage_shift", 8); expect("PGA_STAGE_SHIFT", nullptr, "stage_shift_set", 0);
    expect("PGA_TAIL", "host", "tail", Knobs::host); expect("PGA_TAIL", "anything", "tail", Knobs::par);
    expect("PGA_DP_KERNEL", "", "dp_kernel", Knobs::by_shape); expect("PGA_DP_KERNEL", "", "dp_kernel_set", 1); expect("PGA_DP_KERNEL", "x", "dp_kernel", Knobs::other);
    expect("PGA_KMER_COUNTS_FORM", "lds-wave", "kmer_direct", 0); expect("PGA_KMER_COUNTS_FORM", "lds-wave", "kmer_per_wave", 1);
    expect("PGA_DP_SEG_MIN", "", "dp_seg_min", 16384); expect("PGA_DP_SEG_MIN", "1", "dp_seg_min", 256);
    expect("PGA_PROTEIN_GROUPS_KEY_BITS", "62", "protein_groups_key_bits", 0); expect("PGA_PROTEIN_GROUPS_KEY_BITS", "7x", "protein_groups_key_bits", 0);
    // once per process: the first reading stays
    setenv("PGA_DPW_OCC", "4", 1);
    int64_t v[128]; knobs_process(v);
    setenv("PGA_DPW_OCC", "5", 1);
    int64_t w[128]; const int n = knobs_process(w);
    if (memcmp(v, w, sizeof(int64_t) * n) != 0 || field("dpw_occ") != 5) { printf("process_knobs() moved, or read_knobs() did not\n"); bad++; }
    if (bad) printf("%d checks failed\n", bad); else printf("knobs: all checks passed\n");
    return bad != 0;
}
#endif
