"""Golden archives larger than a committed file may be (1 MiB) are stored as parts: ``<name>.part<k>.npz``.

``save(path, arrays)`` writes ``path`` itself when it fits, else the parts; an array that does not fit one part on its
own is stored flat in pieces (``<key>@<i>``) beside its shape (``<key>@shape``).  ``load(path)`` reads either form and
returns the arrays exactly as they were saved, with the ``.files`` / ``[key]`` surface of ``np.load``."""
import glob
import io
import os

import numpy as np

LIMIT = 1 << 20          # bytes of one committed file
_BUDGET = 900 * 1024     # what a part is filled to (zip headers and compression slack below LIMIT)


def _packed_size(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.tell()


def _pieces(key, arr):
    """(key, array) entries of one array, split flat into pieces that each compress below _BUDGET."""
    if _packed_size({key: arr}) <= _BUDGET:
        return [(key, arr)]
    flat = np.ascontiguousarray(arr).reshape(-1)
    n = 2
    while _packed_size({"x": flat[:-(-flat.size // n)]}) > _BUDGET:
        n *= 2
    step = -(-flat.size // n)
    out = [(f"{key}@shape", np.asarray(arr.shape, dtype=np.int64))]
    out += [(f"{key}@{ii}", flat[pos:pos + step]) for ii, pos in enumerate(range(0, flat.size, step))]
    return out


def _part_paths(path):
    stem = path[:-len(".npz")]
    return sorted(glob.glob(glob.escape(stem) + ".part*.npz"), key=lambda pp: int(pp[len(stem) + 5:-4]))


def save(path, arrays):
    for old in _part_paths(path):
        os.remove(old)
    if os.path.exists(path):
        os.remove(path)
    if _packed_size(arrays) <= _BUDGET:
        np.savez_compressed(path, **arrays)
        return [path]
    parts, cur = [], {}
    for key, arr in arrays.items():
        for kk, vv in _pieces(key, np.asarray(arr)):
            if cur and _packed_size({**cur, kk: vv}) > _BUDGET:
                parts.append(cur)
                cur = {}
            cur[kk] = vv
    parts.append(cur)
    stem = path[:-len(".npz")]
    written = []
    for ii, part in enumerate(parts):
        written.append(f"{stem}.part{ii}.npz")
        np.savez_compressed(written[-1], **part)
        assert os.path.getsize(written[-1]) < LIMIT, written[-1]
    return written


class _Parts:
    def __init__(self, paths):
        self._data = {}
        for pp in paths:
            with np.load(pp) as zz:
                self._data.update({kk: zz[kk] for kk in zz.files})
        shapes = [kk[:-len("@shape")] for kk in self._data if kk.endswith("@shape")]
        for key in shapes:
            shape = tuple(int(vv) for vv in self._data.pop(f"{key}@shape"))
            ii, pieces = 0, []
            while f"{key}@{ii}" in self._data:
                pieces.append(self._data.pop(f"{key}@{ii}"))
                ii += 1
            self._data[key] = np.concatenate(pieces).reshape(shape)
        self.files = list(self._data)

    def __getitem__(self, key):
        return self._data[key].copy()           # like np.load: every read is a fresh array

    def __contains__(self, key):
        return key in self._data


def load(path):
    if os.path.exists(path):
        return np.load(path)
    parts = _part_paths(path)
    if not parts:
        raise FileNotFoundError(path)
    return _Parts(parts)
