"""Proteins as token ids, the parts that need no GPU: the numpy restatement of the rule (tests/protein_tokens_ref.py) on hand-written
proteins, the reference chain over tests/tables_ref.py, what ProteinTokens refuses, and the ctypes mirror of pga_token_opts."""
import ctypes
import itertools
import os
import pickle
import subprocess

import numpy as np
import pytest

from tests.protein_tokens_ref import (AMINO_ACIDS, CODON_COUNTS, protein_tokens_ref, synthetic_contigs, synthetic_proteins,
                                      synthetic_records, vocab_table)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VOCAB = "-" + AMINO_ACIDS + "X*"                     # id = position: '-' 0, A 1 .. Y 20, X 21, * 22
IDS = vocab_table(VOCAB)
HAND = ["MKV", "", "MACDEFGHIK", "M*", "XXW", "MKVLAAGIVR"]


def ids_of(text):
    return [VOCAB.index(c) for c in text]


@pytest.mark.parametrize("bos,eos,max_length", list(itertools.product((None, 30), (None, 31), (None, 5, 9))))
def test_reference_on_hand_written_proteins(bos, eos, max_length):
    s = (bos is not None) + (eos is not None)
    want = []
    for p in HAND:
        r = p if max_length is None else p[:max_length - s]
        want.append(([bos] if bos is not None else []) + ids_of(r) + ([eos] if eos is not None else []))
    if max_length is not None:
        room = max_length - s
        assert any(len(p) > room for p in HAND) and any(len(p) < room for p in HAND)          # n_g > max_length - s, and n_g short of it
    flat, lens, off = protein_tokens_ref(HAND, IDS, bos=bos, eos=eos, max_length=max_length, layout="ragged")
    assert lens.tolist() == [len(w) for w in want] and lens[1] == s                       # n_g = 0: the specials alone
    assert off.tolist() == [0] + list(np.cumsum([len(w) for w in want]))
    assert flat.tolist() == [t for w in want for t in w] and flat.dtype == np.int64
    width = max(len(w) for w in want) + 3
    rows, lens2, none = protein_tokens_ref(HAND, IDS, bos=bos, eos=eos, pad=77, max_length=max_length, layout="padded", width=width, dtype=np.uint8)
    assert none is None and lens2.tolist() == lens.tolist() and rows.shape == (len(HAND), width) and rows.dtype == np.uint8
    for g, w in enumerate(want):
        assert rows[g].tolist() == w + [77] * (width - len(w))
    tight, _, _ = protein_tokens_ref(HAND, IDS, bos=bos, eos=eos, max_length=max_length)
    assert tight.shape == (len(HAND), max(len(w) for w in want))


def test_vocabulary_table_of_the_reference():
    t = vocab_table({"A": 5, "X": 9, "*": 2}, unknown=None)
    assert t[ord("A")] == 5 and t[ord("*")] == 2 and t[ord("C")] == 9 and t[ord("X")] == 9          # no id of its own: X's
    t = vocab_table({"A": 5}, unknown=3)
    assert t[ord("A")] == 5 and t[ord("C")] == 3 and t[ord("*")] == 3


@pytest.mark.parametrize("include_stop", [False, True])
def test_reference_chain_on_the_synthetic_records(include_stop):
    """protein_tokens_ref over tables_ref.translate: lengths follow the coordinates, and the ids decode to the letters."""
    recs, seqs = synthetic_records(), synthetic_contigs()
    assert [r[0] for r in recs] == sorted(r[0] for r in recs) and {r[0] for r in recs} == {0, 1, 2}
    codons = [(e - b + 1) // 3 for _, b, e, _, _, _ in recs]
    assert set(CODON_COUNTS) <= set(codons) and all(1 <= b <= e for _, b, e, _, _, _ in recs)
    assert any(e > len(seqs[c]) for c, _, e, _, _, _ in recs) and all(e <= len(seqs[c]) for c, _, e, _, _, _ in recs if c != 1)
    for c in CODON_COUNTS:
        assert {(st, pb, pe) for (_, b, e, st, pb, pe) in recs if (e - b + 1) // 3 == c} >= {(1, 0, 0), (-1, 0, 0), (1, 1, 1), (-1, 1, 1)}
    prot = synthetic_proteins(include_stop=include_stop)
    assert "X" in "".join(prot) and "*" in "".join(prot) and "M" in [p[0] for p in prot if p]
    flat, lens, off = protein_tokens_ref(prot, IDS, bos=30, eos=31, max_length=40, layout="ragged")
    for g, (c, b, e, st, pb, pe) in enumerate(recs):
        stop_edge = pe if st == 1 else pb
        n = max((e - b + 1) // 3 - (0 if include_stop or stop_edge else 1), 0)
        assert len(prot[g]) == n and lens[g] == 2 + min(n, 38)
        row = flat[off[g]:off[g + 1]]
        assert row[0] == 30 and row[-1] == 31 and "".join(VOCAB[t] for t in row[1:-1]) == prot[g][:38]
    assert sum(n > 38 for n in map(len, prot)) > 5 and sum(n < 38 for n in map(len, prot)) > 5


def test_protein_tokens_refusals_and_pickling():
    from pyrodigal_amd import ProteinTokens
    spec = ProteinTokens(VOCAB, bos=30, eos=31, pad=0, dtype="uint8", layout="ragged", max_length=64, include_stop=True)
    assert list(spec.vocab) == IDS.tolist() and spec.elem_bytes == 1 and spec.specials == 2
    again = pickle.loads(pickle.dumps(spec))
    assert again == spec and hash(again) == hash(spec) and again.vocab == spec.vocab and {spec: 1}[again] == 1
    assert spec != ProteinTokens(VOCAB, bos=30, eos=31, pad=0, dtype="uint8", layout="ragged", max_length=65, include_stop=True)
    as_map = ProteinTokens({c: k for k, c in enumerate(VOCAB)}, bos=30, eos=31, dtype="uint8", layout="ragged", max_length=64, include_stop=True)
    assert as_map == spec
    with pytest.raises(ValueError, match="'W'"):
        ProteinTokens(AMINO_ACIDS.replace("W", "") + "X")
    with pytest.raises(ValueError, match=r"'\*'"):
        ProteinTokens(AMINO_ACIDS + "X", include_stop=True)
    with pytest.raises(ValueError, match="'Z'"):
        ProteinTokens(AMINO_ACIDS + "X", unknown_residue="Z")
    filled = ProteinTokens(AMINO_ACIDS.replace("W", ""), unknown=99, include_stop=True)      # `unknown` stands in for W, X and *
    assert filled.vocab[ord("W")] == 99 and filled.vocab[ord("*")] == 99 and filled.vocab[ord("X")] == 99 and filled.vocab[ord("A")] == 0
    with pytest.raises(ValueError, match="256"):
        ProteinTokens({**{c: k for k, c in enumerate(AMINO_ACIDS + "X")}, "A": 256}, dtype="uint8")
    for field in ("unknown", "bos", "eos", "pad"):
        with pytest.raises(ValueError, match="300"):
            ProteinTokens(VOCAB, dtype="uint8", **{field: 300})
    with pytest.raises(ValueError, match=str(1 << 31)):
        ProteinTokens(VOCAB, dtype="int32", eos=1 << 31)
    ProteinTokens(VOCAB, dtype="int64", eos=1 << 40, bos=-1)
    with pytest.raises(ValueError, match="max_length"):
        ProteinTokens(VOCAB, bos=1, eos=2, max_length=2)
    ProteinTokens(VOCAB, bos=1, eos=2, max_length=3)
    with pytest.raises(ValueError, match="dtype"):
        ProteinTokens(VOCAB, dtype="int16")
    with pytest.raises(ValueError, match="layout"):
        ProteinTokens(VOCAB, layout="jagged")
    with pytest.raises(TypeError):
        ProteinTokens(list(VOCAB))
    with pytest.raises(TypeError):
        ProteinTokens(VOCAB, bos=1.5)


def test_token_lengths_follow_the_coordinates():
    from pyrodigal_amd import ProteinTokens, _cabi
    recs = synthetic_records()
    genes = np.zeros(len(recs), _cabi.GENE_DTYPE)
    for name, col in zip(("contig", "begin", "end", "strand", "partial_begin", "partial_end"), zip(*recs)):
        genes[name] = col
    for include_stop, max_length in ((False, None), (True, None), (False, 18), (True, 40)):
        spec = ProteinTokens(VOCAB, bos=30, max_length=max_length, include_stop=include_stop)
        _, want, _ = protein_tokens_ref(synthetic_proteins(include_stop=include_stop), IDS, bos=30, max_length=max_length, layout="ragged")
        assert spec.lengths(genes).tolist() == want.tolist()


def test_token_opts_mirror_matches_the_header(tmp_path):
    """sizeof and every field offset of pga_token_opts, compiled from the header, against the ctypes mirror."""
    from pyrodigal_amd import _cabi
    fields = [f[0] for f in _cabi.TokenOpts._fields_]
    src = tmp_path / "token_opts.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"pyrodigal_amd.h\"\nint main(void) {\n"
                   "    printf(\"%zu %d %d %lld\\n\", sizeof(pga_token_opts), PGA_TOKENS_RAGGED, PGA_TOKENS_PADDED, (long long)PGA_TOKEN_NONE);\n"
                   + "".join("    printf(\"%%zu\\n\", offsetof(pga_token_opts, %s));\n" % f for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "token_opts"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:4] == [ctypes.sizeof(_cabi.TokenOpts), _cabi.TOKENS_RAGGED, _cabi.TOKENS_PADDED, _cabi.TOKEN_NONE]
    assert got[4:] == [getattr(_cabi.TokenOpts, f).offset for f in fields]
    assert ctypes.sizeof(_cabi.TokenOpts) == 8 + 16 + 16 + 8 + 1024 + 24
