"""Test infrastructure only: the committed golden vectors (tests/golden/transformer_g*.npz).  A golden whose arrays do not fit one
file of PART_LIMIT bytes is stored as <name>.npz plus further parts <name>.p1.npz, <name>.p2.npz, ...; load() merges the parts
into one mapping with np.load's `files`, save() writes them."""
import glob
import io
import os

import numpy as np

PART_LIMIT = 900 << 10


class Golden(dict):
    @property
    def files(self):
        return list(self)


def load(path):
    """path: the first part, <name>.npz."""
    g = Golden()
    for p in [path] + sorted(glob.glob(path[:-len(".npz")] + ".p*.npz"), key=lambda q: int(q[:-len(".npz")].rsplit(".p", 1)[1])):
        with np.load(p) as z:
            for k in z.files:
                assert k not in g, (p, k)
                g[k] = z[k]
    return g


def _compressed_size(key, value):
    buf = io.BytesIO()
    np.savez_compressed(buf, **{key: value})
    return buf.tell()


def save(path, arrays):
    """Writes `arrays` (name -> array) as <name>.npz and as few further parts as keep every file below PART_LIMIT bytes (first fit,
    largest arrays first); parts left over from an earlier save are removed."""
    sizes = {k: _compressed_size(k, v) for k, v in arrays.items()}
    parts = []
    for k in sorted(arrays, key=lambda k: -sizes[k]):
        for part in parts:
            if part[0] + sizes[k] <= PART_LIMIT:
                part[0] += sizes[k]
                part[1].append(k)
                break
        else:
            parts.append([sizes[k], [k]])
    stem = path[:-len(".npz")]
    for old in glob.glob(stem + ".p*.npz"):
        os.remove(old)
    for i, (_, keys) in enumerate(parts):
        np.savez_compressed(path if i == 0 else "%s.p%d.npz" % (stem, i), **{k: arrays[k] for k in keys})
