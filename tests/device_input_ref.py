"""The rule of ``pga_batch_create_device`` (include/pyrodigal_amd.h), restated in numpy for the tests.

Letter j of contig i is f(e), where e is element ``elem_off[i] + j`` of ``data``: an unsigned byte for 1-byte elements, a signed integer
for 4- and 8-byte ones.  Without an alphabet (1-byte elements only) f(e) = e; else f(e) = alphabet[e] for 0 <= e < len(alphabet) and 'N'
for every other value, negative ones included."""
import numpy as np


def pack_reference(data, elem_off, lens, alphabet):
    """``data``: a numpy array (any shape: it is read flat, in C order) of dtype uint8 / int8 / int32 / int64; ``alphabet``: ``None`` or
    ``bytes``.  Returns the letters of every contig, a ``bytes`` each."""
    flat = np.ascontiguousarray(data).reshape(-1)
    if flat.dtype.itemsize == 1:
        flat = flat.view(np.uint8)
    elif flat.dtype not in (np.dtype("<i4"), np.dtype("<i8")):
        raise TypeError("elements of %s" % flat.dtype)
    if alphabet is None and flat.dtype.itemsize != 1:
        raise ValueError("token ids need an alphabet")
    table = None if alphabet is None else np.frombuffer(bytes(alphabet), np.uint8)
    out = []
    for o, n in zip(elem_off, lens):
        o, n = int(o), int(n)
        if o < 0 or n < 0 or o + n > flat.size:
            raise ValueError("elements [%d, %d + %d) do not lie in the %d elements of the data" % (o, o, n, flat.size))
        e = flat[o:o + n].astype(np.int64)
        if table is None:
            out.append(e.astype(np.uint8).tobytes())
            continue
        ok = (e >= 0) & (e < table.size)
        letters = np.full(n, ord("N"), np.uint8)
        if table.size:
            letters[ok] = table[e[ok]]
        out.append(letters.tobytes())
    return out
