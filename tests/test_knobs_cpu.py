"""The run-time knobs (pyrodigal_amd/csrc/knobs.h), built host-only through tests/knobs_shim.cpp: every PGA_* variable against a
restatement of the rule it had at the site that used to parse it, the once-per-process subset, and two checks of the source text --
nothing else under csrc reads the environment, and the knob table of INTEGRATION.md names exactly the knobs of knobs.h."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "knobs_shim.cpp")
CSRC = os.path.join(ROOT, "pyrodigal_amd", "csrc")
HDR = os.path.join(CSRC, "knobs.h")
LIB = os.path.join(HERE, "libknobs_shim.so")

TAIL = {"par": 0, "device": 1, "host": 2}
KERNEL = {"by_shape": 0, "wave": 1, "tree1": 2, "tree3": 3, "scan": 4, "other": 5}


def build_shim():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", LIB, SRC], check=True)
    L = ctypes.CDLL(LIB)
    L.knobs_field_names.restype = ctypes.c_char_p
    return L


@pytest.fixture(scope="module")
def shim():
    return build_shim()


def fields(L, call="knobs_read"):
    names = L.knobs_field_names().decode().rstrip(",").split(",")
    out = (ctypes.c_int64 * 128)()
    n = getattr(L, call)(out)
    assert n == len(names)
    return dict(zip(names, out[:n]))


def read_with(L, name, value):
    """the knobs with `name` set to `value` (None: unset) and no other PGA_* variable in the environment"""
    saved = {k: v for k, v in os.environ.items() if k.startswith("PGA_")}
    for k in saved:
        del os.environ[k]
    try:
        if value is not None:
            os.environ[name] = value
        return fields(L)
    finally:
        os.environ.pop(name, None)
        os.environ.update(saved)


# ---- the restatement: what each site did with getenv(X) --------------------------------------------------------------------
def atoi(s):
    m = re.match(r"[ \t\n\v\f\r]*([+-]?[0-9]+)", s)
    return int(m.group(1)) if m else 0


def present(field):                                   # getenv(X) != nullptr
    return lambda v: {field: int(v is not None)}


def unless_zero(field):                               # !(getenv(X) && atoi(getenv(X)) == 0)
    return lambda v: {field: int(not (v is not None and atoi(v) == 0))}


def non_zero(field):                                  # getenv(X) && atoi(getenv(X))
    return lambda v: {field: int(v is not None and atoi(v) != 0)}


def clamped(field, lo, hi, dflt):                     # getenv(X) ? max(lo, min(hi, atoi(..))) : dflt
    return lambda v: {field: dflt if v is None else max(lo, min(hi, atoi(v)))}


def in_range_or_default(field, lo, hi, dflt):         # out of range: the default, not the nearest end
    return lambda v: {field: dflt if v is None or not lo <= atoi(v) <= hi else atoi(v)}


def one_of_or(field, allowed, dflt):
    return lambda v: {field: atoi(v) if v is not None and atoi(v) in allowed else dflt}


def env_int(v, dflt):                                 # dp.hip: (e && *e) ? atoi(e) : dflt -- the empty string counts as unset
    return atoi(v) if v else dflt


def dp_kernel(v):
    # pga_dp_use_wave: a non-empty value decides (== "wave"), else the launch shape; pga_dp_plan and the segment-wave choice: set at all;
    # pga_launch_dp: "scan", "tree1", "tree3" by strcmp
    word = "by_shape" if not v else v if v in ("wave", "tree1", "tree3", "scan") else "other"
    return {"dp_kernel_set": int(v is not None), "dp_kernel": KERNEL[word]}


def kmer_form(v):
    direct = per_wave = -1
    if v is not None:
        direct = 1 if "direct" in v else 0 if "lds" in v else -1
        per_wave = 1 if "wave" in v else 0 if "group" in v else -1
    return {"kmer_direct": direct, "kmer_per_wave": per_wave}


def key_bits(v):
    if v is None:
        return {"protein_groups_key_bits": 61}
    m = re.fullmatch(r"[ \t\n\v\f\r]*[+-]?[0-9]+", v)         # strtol reads the whole string
    return {"protein_groups_key_bits": int(v) if m and 1 <= int(v) <= 61 else 0}


EMPTY_AND_WORD = ["", "abc"]
FLAG = [None, "0", "1", "2", "-1"] + EMPTY_AND_WORD        # for the presence tests and the 0-means-off switches alike

# name -> (rule, values); every list holds: unset, the default spelled out, each accepted value or both ends of the range, one value
# just outside each end, the empty string, a non-number
RULES = {
    "PGA_TIMING": (present("timing"), FLAG),
    "PGA_FAULT_CONTIG_LEN": (lambda v: {"fault_contig_len_set": int(v is not None), "fault_contig_len": atoi(v) if v is not None else 0},
                             [None, "0", "20000", "-1", "3000000000"] + EMPTY_AND_WORD),
    "PGA_PAGEABLE_RESULTS": (present("pageable_results"), FLAG),
    "PGA_CACHE_GB": (lambda v: {"cache_gb": 16 if v is None else max(0, atoi(v))}, [None, "16", "0", "-1", "1", "64"] + EMPTY_AND_WORD),
    "PGA_UPLOAD_TURNS": (unless_zero("upload_turns"), FLAG),
    "PGA_MALLOPT": (unless_zero("mallopt"), FLAG),
    "PGA_DP_SEG_HEIGHT": (in_range_or_default("dp_seg_height", 2, 24, 4), [None, "4", "1", "2", "24", "25"] + EMPTY_AND_WORD),
    "PGA_DPW_OCC": (in_range_or_default("dpw_occ", 4, 6, 6), [None, "6", "3", "4", "5", "7"] + EMPTY_AND_WORD),
    "PGA_PRINT_BUFFERS": (present("print_buffers"), FLAG),
    "PGA_FASTA_NO_MMAP": (present("fasta_no_mmap"), FLAG),
    "PGA_FASTA_THREADS": (lambda v: {"fasta_threads": 0 if v is None else max(1, atoi(v))}, [None, "1", "0", "-3", "16", "64"] + EMPTY_AND_WORD),
    "PGA_STAGE_FULL": (present("stage_full"), FLAG),
    "PGA_STAGE_SHIFT": (lambda v: {"stage_shift_set": int(v is not None), "stage_shift": 1 if v is None else max(1, min(8, atoi(v)))},
                        [None, "1", "0", "5", "8", "9", "99"] + EMPTY_AND_WORD),
    "PGA_EXTRACT_C": (clamped("extract_c", 0, 4, 4), [None, "4", "-1", "0", "1", "5", "9"] + EMPTY_AND_WORD),
    "PGA_EXTRACT_POOL": (clamped("extract_pool", 0, 128, 128), [None, "128", "-1", "0", "129"] + EMPTY_AND_WORD),
    "PGA_CS_LDS": (unless_zero("cs_lds"), FLAG),
    "PGA_CS_TASK_NODES": (in_range_or_default("cs_task_nodes", 256, 8192, 5120), [None, "5120", "255", "256", "8192", "8193"] + EMPTY_AND_WORD),
    "PGA_CS_WAVE": (lambda v: {"cs_wave": atoi(v) if v is not None and atoi(v) >= 64 else 2048}, [None, "2048", "63", "64", "100000"] + EMPTY_AND_WORD),
    "PGA_CS_QCLASSES": (lambda v: {"cs_qclasses": 4 if v is not None and atoi(v) == 4 else 3}, [None, "3", "4", "2", "5"] + EMPTY_AND_WORD),
    "PGA_CS_PROFILE": (present("cs_profile"), FLAG),
    "PGA_SS_STARTS_ONLY": (unless_zero("ss_starts_only"), FLAG),
    "PGA_SS_MM": (unless_zero("ss_mm"), FLAG),
    "PGA_SS_MM_TILE": (one_of_or("ss_mm_tile", (256, 512, 1024), 1024), [None, "1024", "256", "512", "300", "255", "1025", "2048"] + EMPTY_AND_WORD),
    "PGA_SS_MODELS_PER_PASS": (in_range_or_default("ss_models_per_pass", 1, 512, 512), [None, "512", "0", "1", "513"] + EMPTY_AND_WORD),
    "PGA_SS_FULL_STOPS": (present("ss_full_stops"), FLAG),
    "PGA_SS_PROFILE": (present("ss_profile"), FLAG),
    "PGA_OVL_SEARCH": (present("ovl_search"), FLAG),
    "PGA_DP_KERNEL": (dp_kernel, [None, "wave", "tree1", "tree3", "scan", "Wave", "waves", "", "abc", "0"]),
    "PGA_DP_WAVES": (one_of_or("dp_waves", (1, 4, 16), 0), [None, "1", "4", "16", "8", "0", "17"] + EMPTY_AND_WORD),
    "PGA_DP_PROFILE": (present("dp_profile"), FLAG),
    "PGA_DP_SEG": (lambda v: {"dp_seg": int(env_int(v, 1) != 0)}, FLAG),
    "PGA_DP_SEG_MIN": (lambda v: {"dp_seg_min": max(256, env_int(v, 16384))}, [None, "16384", "255", "256", "257", "1000000"] + EMPTY_AND_WORD),
    "PGA_DP_SEG_WARM": (lambda v: {"dp_seg_warm": max(64, env_int(v, 4096))}, [None, "4096", "63", "64", "65"] + EMPTY_AND_WORD),
    "PGA_DP_SEG_LEN": (lambda v: {"dp_seg_len_set": int(env_int(v, 0) > 0), "dp_seg_len": env_int(v, 0)}, [None, "0", "-1", "1", "4096"] + EMPTY_AND_WORD),
    "PGA_DP_SEG_SLOTS": (lambda v: {"dp_seg_slots": max(64, env_int(v, 256) - 4)}, [None, "256", "67", "68", "69", "1024"] + EMPTY_AND_WORD),
    "PGA_DP_SEG_WSLOTS": (lambda v: {"dp_seg_wslots": max(64, env_int(v, 4096))}, [None, "4096", "63", "64", "65"] + EMPTY_AND_WORD),
    "PGA_DP_SEG_WAVE": (lambda v: {"dp_seg_wave_set": int(v is not None), "dp_seg_wave": int(v is not None and atoi(v) != 0)}, FLAG),
    "PGA_DP_SEG_WAVE_MIN": (lambda v: {"dp_seg_wave_min": 2500000 if v is None else atoi(v)}, [None, "2500000", "0", "-1", "5000000000"] + EMPTY_AND_WORD),
    "PGA_DP_SEG_READBACK": (unless_zero("dp_seg_readback"), FLAG),
    "PGA_DP_SEG_DEBUG": (present("dp_seg_debug"), FLAG),
    "PGA_DP_NO_ORDER": (present("dp_no_order"), FLAG),
    "PGA_DP_XCD": (unless_zero("dp_xcd"), FLAG),
    "PGA_DPW_SCHED": (unless_zero("dpw_sched"), FLAG),                 # e ? atoi(e) != 0 : true -- the same thing
    "PGA_DPW_SCHED_MISS": (non_zero("dpw_sched_miss"), FLAG),
    "PGA_DPW_SCHED_DEBUG": (present("dpw_sched_debug"), FLAG),
    "PGA_DPW_TOPO_WALK": (non_zero("dpw_topo_walk"), FLAG),
    "PGA_DPW_TOPO_LDS": (unless_zero("dpw_topo_lds"), FLAG),
    "PGA_TAIL": (lambda v: {"tail": TAIL[v] if v in ("host", "device") else TAIL["par"]}, [None, "par", "host", "device", "Host", "hosts", "", "abc", "0"]),
    "PGA_FULL_GATHER": (present("full_gather"), FLAG),
    "PGA_GATHER_ALL_DP": (present("gather_all_dp"), FLAG),
    "PGA_TP_STEPS": (present("tp_steps"), FLAG),
    "PGA_TP_JUMP8": (unless_zero("tp_jump8"), FLAG),
    "PGA_TP_EXTRACT_ONE": (present("tp_extract_one"), FLAG),
    "PGA_TWEAK_SLOTS": (present("tweak_slots"), FLAG),
    "PGA_KMER_COUNTS_FORM": (kmer_form, [None, "lds", "direct", "wave", "group", "lds-wave", "direct-group", "direct,lds", "", "abc", "0"]),
    "PGA_PROTEIN_GROUPS_KEY_BITS": (key_bits, [None, "61", "1", "0", "62", "-1", " 7", "7 ", "7x", "", "abc"]),
}


def knob_names_in_header():
    return set(re.findall(r"PGA_[A-Z0-9_]+", open(HDR).read()))


def test_every_knob_of_the_header_has_a_rule():
    assert knob_names_in_header() == set(RULES)


@pytest.mark.parametrize("name", sorted(RULES))
def test_knob_rule(shim, name):
    rule, values = RULES[name]
    baseline = read_with(shim, name, None)
    for value in values:
        got = read_with(shim, name, value)
        want = dict(baseline)
        want.update(rule(value))
        assert got == want, (name, value, {k: (got[k], want[k]) for k in got if got[k] != want[k]})


def test_defaults(shim):
    d = read_with(shim, "PGA_TIMING", None)
    want = {"cache_gb": 16, "upload_turns": 1, "mallopt": 1, "dp_seg_height": 4, "dpw_occ": 6, "fasta_threads": 0, "stage_shift": 1, "extract_c": 4,
            "extract_pool": 128, "cs_lds": 1, "cs_task_nodes": 5120, "cs_wave": 2048, "cs_qclasses": 3, "ss_starts_only": 1, "ss_mm": 1,
            "ss_mm_tile": 1024, "ss_models_per_pass": 512, "dp_kernel": KERNEL["by_shape"], "dp_waves": 0, "dp_seg": 1, "dp_seg_min": 16384,
            "dp_seg_warm": 4096, "dp_seg_slots": 252, "dp_seg_wslots": 4096, "dp_seg_wave_min": 2500000, "dp_seg_readback": 1, "dp_xcd": 1,
            "dpw_sched": 1, "dpw_topo_lds": 1, "tail": TAIL["par"], "tp_jump8": 1, "kmer_direct": -1, "kmer_per_wave": -1, "protein_groups_key_bits": 61}
    assert {k: d[k] for k in want} == want
    assert all(v == 0 for k, v in d.items() if k not in want), {k: v for k, v in d.items() if k not in want and v}


ONCE = {"PGA_CACHE_GB": ("cache_gb", "3", "5"), "PGA_UPLOAD_TURNS": ("upload_turns", "0", "1"), "PGA_MALLOPT": ("mallopt", "0", "1"),
        "PGA_DP_SEG_HEIGHT": ("dp_seg_height", "8", "12"), "PGA_DPW_OCC": ("dpw_occ", "4", "5")}


def once_per_process_child():
    L = build_shim()
    for name, (_, first, _) in ONCE.items():
        os.environ[name] = first
    before = fields(L, "knobs_process")
    for name, (_, _, second) in ONCE.items():
        os.environ[name] = second
    after, fresh = fields(L, "knobs_process"), fields(L)
    for name, (field, first, second) in ONCE.items():
        assert before[field] == after[field] == int(first), (name, before[field], after[field])
        assert fresh[field] == int(second), (name, fresh[field])
    assert before == after
    print("once-per-process ok")


def test_once_per_process_knobs_keep_their_first_reading(shim):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PGA_")}
    r = subprocess.run([sys.executable, "-c", "import test_knobs_cpu as t; t.once_per_process_child()"], cwd=HERE, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0 and "once-per-process ok" in r.stdout, r.stdout + r.stderr


# ---- the source text ---------------------------------------------------------------------------------------------------------
def test_only_knobs_h_reads_the_environment():
    readers = [n for n in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, n)) and n != "knobs.h"
               and "getenv" in open(os.path.join(CSRC, n), errors="replace").read()]
    assert readers == []


def knob_names_in_integration_table():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = text.split("## Run-time knobs and diagnostics", 1)[1].split("\n## ", 1)[0]
    rows = [line for line in section.splitlines() if line.startswith("| `PGA_")]
    return set(n for line in rows for n in re.findall(r"PGA_[A-Z0-9_]+", line.split("|")[1]))


def test_integration_table_names_the_knobs_of_the_header():
    assert knob_names_in_integration_table() == knob_names_in_header()
