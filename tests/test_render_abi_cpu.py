"""CPU-only checks of the render boundary: the ctypes mirrors of pga_render_opts / pga_render_result against the header, and the
argument checks Context.render_genes makes before it touches a device (format names, GenBank dates and tables)."""
import ctypes
import datetime
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_render_struct_layout_matches_the_header(tmp_path):
    from pyrodigal_amd import _cabi
    src = tmp_path / "render_sizes.c"
    src.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "pyrodigal_amd.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\\n",
           sizeof(pga_render_opts), offsetof(pga_render_opts, fallback_margin), offsetof(pga_render_opts, gbk_division),
           offsetof(pga_render_opts, gbk_date), offsetof(pga_render_opts, gbk_version), offsetof(pga_render_opts, gbk_translation_table),
           offsetof(pga_render_opts, gbk_strict), offsetof(pga_render_opts, sco_header),
           sizeof(pga_text), sizeof(pga_render_result), offsetof(pga_render_result, text), offsetof(pga_render_result, t_kernels_ms),
           sizeof(pga_params), PGA_RENDER_GBK, PGA_RENDER_SCO, PGA_NODES_DEVICE);
    return 0;
}
""")
    exe = tmp_path / "render_sizes"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    O, T, R = _cabi.RenderOpts, _cabi.Text, _cabi.RenderResult
    assert got == [ctypes.sizeof(O), O.fallback_margin.offset, O.gbk_division.offset, O.gbk_date.offset, O.gbk_version.offset,
                   O.gbk_translation_table.offset, O.gbk_strict.offset, O.sco_header.offset,
                   ctypes.sizeof(T), ctypes.sizeof(R), R.text.offset, R.t_kernels_ms.offset,
                   ctypes.sizeof(_cabi.Params), 8, 16, _cabi.NODES_DEVICE]
    # the fields that were there before keep their offsets; five texts and five timings, in PGA_RENDER_* bit order
    assert O.fallback_margin.offset == 80 and R.t_kernels_ms.offset == 8 + 5 * ctypes.sizeof(T)
    assert _cabi.RENDER_FORMATS == ("gff", "faa", "fna", "gbk", "scores")


class _Nothing:
    """Stands in for the context, batch and result: every check below must fail before any of them is used."""

    def __getattr__(self, name):
        raise AssertionError("the device layer was reached (%s)" % name)


def render(formats, **kw):
    from pyrodigal_amd import _cabi
    return _cabi._render_genes(_Nothing(), _Nothing(), _Nothing(), ["a"], formats, **kw)


def test_unknown_format_names():
    with pytest.raises(ValueError, match="unknown format 'genbank'"):
        render(("gff", "genbank"))
    with pytest.raises(ValueError, match="expected one of gff, faa, fna, gbk, scores"):
        render("score")
    with pytest.raises(TypeError, match="unexpected option"):
        render({"scores": {"width": 3}})
    with pytest.raises(TypeError, match="unexpected option"):
        render("gbk", nonsense=1)


@pytest.mark.parametrize("date", ["16-OCT-26", 20261016, datetime.time(1, 2)])
def test_bad_genbank_dates(date):
    with pytest.raises(TypeError, match="Expected datetime.date, found %s" % type(date).__name__):
        render("gbk", date=date)
    with pytest.raises(TypeError, match="Expected datetime.date"):
        render({"gbk": {"date": date}})


@pytest.mark.parametrize("table", [0, 7, 8, 34, "11"])
def test_bad_genbank_translation_tables(table):
    with pytest.raises(ValueError, match="not a valid translation table index"):
        render({"gbk": {"translation_table": table}})


def test_genbank_options_resolved_as_write_genbank_does():
    from pyrodigal_amd import _cabi
    o = _cabi._render_formats(("gbk", "scores"), {})
    assert o["gbk"]["division"] == "BCT" and o["gbk"]["date"] == datetime.date.today()
    assert o["gbk"]["translation_table"] is None and o["gbk"]["strict_translation"] is True
    assert o["scores"] == {"header": True}
    d = datetime.datetime(2026, 1, 2, 3, 4)             # a datetime is a date, as for write_genbank
    o = _cabi._render_formats({"gbk": {"date": d, "translation_table": 4}, "scores": {"header": False}}, {})
    assert o["gbk"]["date"] is d and o["gbk"]["translation_table"] == 4 and o["scores"]["header"] is False
    # options shared by name: `header` reaches GFF and scores, `strict_translation` protein FASTA and GenBank
    o = _cabi._render_formats(("gff", "scores", "faa", "gbk"), {"header": False, "strict_translation": False})
    assert not o["gff"]["header"] and not o["scores"]["header"]
    assert not o["faa"]["strict_translation"] and not o["gbk"]["strict_translation"]


def test_want_nodes_values():
    from pyrodigal_amd import _cabi
    assert [_cabi._want_nodes(x) for x in (False, True, 0, 1, "device")] == [0, 1, 0, 1, 2]
    with pytest.raises(ValueError, match="device"):
        _cabi._want_nodes("host")
