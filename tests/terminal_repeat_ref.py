"""Direct terminal repeats, the rule of DESIGN.md 4.12 in plain Python: the longest r for which the first r letters of a record are
also its last r, the low-complexity filter, and the record without the second copy.  Written from the definition, letter by letter;
the device (tests/test_terminal_repeat_gpu.py) must agree with it on every contig."""

DIGIT = {"A": 0, "G": 1, "C": 2, "T": 3}          # digit_of: either case; everything else is unknown and matches nothing
DEFAULTS = dict(min_length=20, max_length=65536, max_base_percent=75)


def letters_match(a, b):
    a, b = chr(a).upper(), chr(b).upper()
    return a in DIGIT and a == b


def _side(unknown):
    t = bytearray([unknown]) * 256
    for ch in b"ACGT":
        t[ch] = ch
        t[ch + 32] = ch
    return bytes(t)


_SIDE = (_side(ord("<")), _side(ord(">")))


def check_params(min_length, max_length, max_base_percent):
    if not (1 <= min_length <= max_length <= 1048576) or not (25 <= max_base_percent <= 100):
        raise ValueError("bad terminal-repeat parameters")


def find_match(seq, min_length=20, max_length=65536):
    """The largest r in min_length .. min(max_length, L // 2) with S[j] matching S[L - r + j] for every j < r; 0 when there is none."""
    L = len(seq)
    W = min(max_length, L // 2)
    # letters_match over whole slices: the four bases read as their upper case, every other letter as something that differs between
    # the two ends and from every base
    head, tail = bytes(seq).translate(_SIDE[0]), bytes(seq).translate(_SIDE[1])
    for r in range(W, min_length - 1, -1):
        if head[:r] == tail[L - r:]:
            return r
    return 0


def low_complexity(seq, match, max_base_percent=75):
    up = seq[:match].upper()
    c = max(up.count(b) for b in (b"A", b"G", b"C", b"T"))
    return 100 * c > max_base_percent * match


def terminal_repeat(seq, min_length=20, max_length=65536, max_base_percent=75):
    """(match, trim, T): T = seq[:L - trim] is what the finder calls as a circle when trim > 0."""
    check_params(min_length, max_length, max_base_percent)
    seq = bytes(seq)
    match = find_match(seq, min_length, max_length)
    trim = 0 if match and low_complexity(seq, match, max_base_percent) else match
    return match, trim, seq[:len(seq) - trim]


def clip_regions(regions, new_length):
    """The caller's regions of a trimmed record: clipped to [0, new_length), empty ones dropped."""
    out = [(b, min(e, new_length)) for b, e in regions]
    return [(b, e) for b, e in out if b < e]


def status(match, trim):
    return "trimmed" if trim > 0 else "low_complexity" if match > 0 else "none"
