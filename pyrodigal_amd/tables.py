"""Choice of a genome's translation table by coding density.

Pure Python: importing this module does not load the HIP library, so the command line, the CPU tests and the Cython layer
(``GeneFinder.select_translation_table``) share one definition of the rule.

The coding density of a genome under a table is the fraction of its bases that lie inside at least one gene called in single mode
with a model trained on that genome under that table.  A candidate other than the default qualifies when it covers more than
``min_gain`` more of the genome than the default does and more than ``min_density`` of it (both strict); the qualifying candidate
with the highest density wins, the one listed first on a tie, and the default table when none qualifies.  With the defaults this is
the usual test for genomes that read TGA as tryptophan: 11 unless 4 covers more than 5 points more and over 70 %.
"""
import numbers
import types

__all__ = ["DEFAULT_CANDIDATES", "DEFAULT_MIN_GAIN", "DEFAULT_MIN_DENSITY", "TRANSLATION_TABLES", "NCBI_CODES", "check_candidates",
           "check_thresholds", "coding_density", "choose_table", "TableSelection"]

# the NCBI genetic codes the reference knows (lib.pyx TRANSLATION_TABLES, restated so that nothing here needs a compiled module)
TRANSLATION_TABLES = frozenset(set(range(1, 7)) | set(range(9, 17)) | set(range(21, 27)) | {29, 30, 32, 33})

# NCBI genetic codes: amino acids of the 64 codons in TCAG order (first base slowest).  Table numbers as in
# the reference (_translation.h; TRANSLATION_TABLES above).  `GeneFinder` translates with them, `KmerCounts.codon_bins` bins by them.
NCBI_CODES = {
    1: "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    2: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSS**VVVVAAAADDEEGGGG",
    3: "FFLLSSSSYY**CCWWTTTTPPPPHHQQRRRRIIMMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    4: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    5: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSSSSVVVVAAAADDEEGGGG",
    6: "FFLLSSSSYYQQCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    9: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNNKSSSSVVVVAAAADDEEGGGG",
    10: "FFLLSSSSYY**CCCWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    11: "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    12: "FFLLSSSSYY**CC*WLLLSPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    13: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNKKSSGGVVVVAAAADDEEGGGG",
    14: "FFLLSSSSYYY*CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNNKSSSSVVVVAAAADDEEGGGG",
    15: "FFLLSSSSYY*QCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    16: "FFLLSSSSYY*LCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    21: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIMMTTTTNNNKSSSSVVVVAAAADDEEGGGG",
    22: "FFLLSS*SYY*LCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    23: "FF*LSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    24: "FFLLSSSSYY**CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSSKVVVVAAAADDEEGGGG",
    25: "FFLLSSSSYY**CCGWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    26: "FFLLSSSSYY**CC*WLLLAPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    29: "FFLLSSSSYYYYCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    30: "FFLLSSSSYYEECC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    32: "FFLLSSSSYY*WCC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG",
    33: "FFLLSSSSYYY*CCWWLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSSKVVVVAAAADDEEGGGG",
}

DEFAULT_CANDIDATES = (11, 4)
DEFAULT_MIN_GAIN = 0.05
DEFAULT_MIN_DENSITY = 0.7
MAX_CANDIDATES = 4          # the distinct translation tables one device call holds


def check_candidates(candidates):
    """The candidate tables as a tuple of ints: 1 to 4 distinct valid tables, the first one the default (else ValueError)."""
    if isinstance(candidates, (str, bytes)) or not hasattr(candidates, "__iter__"):
        raise ValueError("`candidates` must be a sequence of translation tables, not %r" % (candidates,))
    out = []
    for t in candidates:
        if isinstance(t, bool) or not isinstance(t, numbers.Integral):
            raise ValueError("%r is not a valid translation table index" % (t,))
        t = int(t)
        if t not in TRANSLATION_TABLES:
            raise ValueError("%d is not a valid translation table index" % t)
        if t in out:
            raise ValueError("translation table %d is listed twice in `candidates`" % t)
        out.append(t)
    if not out:
        raise ValueError("`candidates` is empty")
    if len(out) > MAX_CANDIDATES:
        raise ValueError("at most %d candidate tables, not %d" % (MAX_CANDIDATES, len(out)))
    return tuple(out)


def check_thresholds(min_gain, min_density):
    """Both thresholds as floats in [0, 1] (else ValueError)."""
    out = []
    for name, v in (("min_gain", min_gain), ("min_density", min_density)):
        v = float(v)
        if not (0.0 <= v <= 1.0):           # NaN fails too
            raise ValueError("`%s` must lie in [0, 1], not %r" % (name, v))
        out.append(v)
    return tuple(out)


def coding_density(coding_bases, length):
    """``coding_bases / length`` as one double division of the two integers (what the host and the device both compute)."""
    return float(int(coding_bases)) / float(int(length)) if length else 0.0


def choose_table(density, candidates=DEFAULT_CANDIDATES, min_gain=DEFAULT_MIN_GAIN, min_density=DEFAULT_MIN_DENSITY):
    """The rule: ``density`` maps every candidate table to its coding density; returns the chosen table."""
    cands = check_candidates(candidates)
    min_gain, min_density = check_thresholds(min_gain, min_density)
    default = cands[0]
    best = None
    for t in cands[1:]:
        d = density[t]
        if d - density[default] > min_gain and d > min_density and (best is None or d > density[best]):
            best = t
    return default if best is None else best


class TableSelection:
    """The translation table chosen for one genome (``GeneFinder.select_translation_table``), read-only.

    ``translation_table``: the chosen table; ``training_info``: the model trained on the genome with it; ``coding_density`` and
    ``coding_bases``: read-only mappings from every candidate table to the density / the bases inside genes; ``length``: the
    genome's bases (the sum of its contigs' lengths, N included)."""
    __slots__ = ("_table", "_tinf", "_density", "_bases", "_length")

    def __init__(self, translation_table, training_info, coding_bases, length):
        object.__setattr__(self, "_table", int(translation_table))
        object.__setattr__(self, "_tinf", training_info)
        object.__setattr__(self, "_bases", types.MappingProxyType({int(t): int(n) for t, n in coding_bases.items()}))
        object.__setattr__(self, "_density", types.MappingProxyType({t: coding_density(n, length) for t, n in self._bases.items()}))
        object.__setattr__(self, "_length", int(length))

    def __setattr__(self, name, value):
        raise AttributeError("TableSelection is read-only")

    def __delattr__(self, name):
        raise AttributeError("TableSelection is read-only")

    @property
    def translation_table(self):
        return self._table

    @property
    def training_info(self):
        return self._tinf

    @property
    def coding_density(self):
        return self._density

    @property
    def coding_bases(self):
        return self._bases

    @property
    def length(self):
        return self._length

    def __repr__(self):
        dens = ", ".join("%d: %.4f" % (t, d) for t, d in self._density.items())
        return "TableSelection(translation_table=%d, coding_density={%s}, length=%d)" % (self._table, dens, self._length)
