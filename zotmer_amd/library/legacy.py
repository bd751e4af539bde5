"""
The reference's older container (zotmer/library/container/__init__.py, container/vectors.py, container/std.py): the file format
of the k-mer index of `zot mlst` (library/index.py:117-125).  Read and written here in pure Python, so that an index built by
either program opens in the other.

A container is a ZIP file (allowZip64).  Member `__meta__` is a pickled dict, stored (container/__init__.py:107-113).  Every
other member is a vector, deflated, laid out by container/vectors.py:67-122: a run of blocks, one per 65 536 items; a block is
an 8-byte `unsigned long` byte length (struct 'L', native: little-endian on every machine the reference ran on) followed by the
items, raw (array.tostring()).  writeGeneric always writes a last block, also when it is empty -- after an exact multiple of
65 536 items, and for no items at all (vectors.py:85-88).  The reader stops after the number of items the meta names, or at the
end of the member (vectors.py:108-122).

Here the items are written explicitly little-endian and the length word as '<Q'; `__meta__` is written with pickle protocol 2
(which Python 2's cPickle reads) and read by an Unpickler that refuses every global: the reference's meta holds only dict, str,
int and list, so an index file can never run code.
"""
import io
import pickle
import struct
import zipfile
import zlib

import numpy as np

BLOCK_ITEMS = 65536                                  # vectors.py:11
META = "__meta__"
_DTYPES = {8: np.dtype("<u8"), 4: np.dtype("<u4"), 2: np.dtype("<u2")}


class LegacyError(IOError):
    pass


# ---- vectors ------------------------------------------------------------------------------------------------------------

def pack_vector(values, width):
    """the bytes of a member as writeGeneric writes them (vectors.py:67-89); width = bytes per item (8, 4 or 2)"""
    a = np.ascontiguousarray(values, dtype=_DTYPES[width])
    out = []
    full = a.size - a.size % BLOCK_ITEMS
    for lo in range(0, full, BLOCK_ITEMS):
        out.append(struct.pack("<Q", BLOCK_ITEMS * width))
        out.append(a[lo:lo + BLOCK_ITEMS].tobytes())
    tail = a[full:]                                  # always written, also when it is empty
    out.append(struct.pack("<Q", tail.size * width))
    out.append(tail.tobytes())
    return b"".join(out)


def unpack_vector(data, width, n, name="?"):
    """the first n items of a member's bytes (readGeneric, vectors.py:103-122).  A trailing empty block, or anything after the
    n-th item's block, is never looked at; a member that ends before n items is an error that names it."""
    dt = _DTYPES[width]
    parts, have, pos = [], 0, 0
    while have < n:
        if pos + 8 > len(data):
            raise LegacyError("member %r is truncated: %d of %d items" % (name, have, n))
        (length,) = struct.unpack_from("<Q", data, pos)
        pos += 8
        if length % width or pos + length > len(data):
            raise LegacyError("member %r is truncated: a block of %d bytes at byte %d of %d" % (name, length, pos, len(data)))
        parts.append(np.frombuffer(data, dtype=dt, count=length // width, offset=pos))
        have += length // width
        pos += length
    out = np.concatenate(parts) if parts else np.empty(0, dtype=dt)
    if have != n:
        raise LegacyError("member %r holds %d items in the blocks that should hold %d" % (name, have, n))
    return out.astype(dt.newbyteorder("="), copy=False)


# ---- the meta -----------------------------------------------------------------------------------------------------------

class _NoGlobals(pickle.Unpickler):
    def find_class(self, module, name):
        raise LegacyError("the meta names %s.%s: only dict, str, int and list are read" % (module, name))


def load_meta(data):
    try:
        meta = _NoGlobals(io.BytesIO(data), encoding="latin-1").load()
    except LegacyError:
        raise
    except Exception as e:
        raise LegacyError("member %r is not a pickle: %s" % (META, e))
    if not isinstance(meta, dict):
        raise LegacyError("member %r is not a dict" % META)
    return meta


def dump_meta(meta):
    return pickle.dumps(meta, protocol=2)


# ---- the container ------------------------------------------------------------------------------------------------------

def write_container(path, meta, vectors):
    """vectors: [(member name, values, bytes per item)] in the order they are written; `__meta__` goes last, stored
    (container/__init__.py:107-113)"""
    with zipfile.ZipFile(path, "w", allowZip64=True) as z:
        for name, values, width in vectors:
            z.writestr(name, pack_vector(values, width), compress_type=zipfile.ZIP_DEFLATED)
        z.writestr(META, dump_meta(meta), compress_type=zipfile.ZIP_STORED)


class Reader:
    """container(path, 'r'): .meta, and vector(name, width, n)"""

    def __init__(self, path):
        self.path = path
        try:
            self.z = zipfile.ZipFile(path, "r", allowZip64=True)
        except zipfile.BadZipFile as e:
            raise LegacyError("%s: not a container: %s" % (path, e))
        self.meta = load_meta(self.member(META))

    def member(self, name):
        try:
            return self.z.read(name)
        except KeyError:
            raise LegacyError("%s: member %r is missing" % (self.path, name))
        except (zipfile.BadZipFile, EOFError, zlib.error) as e:
            raise LegacyError("%s: member %r is damaged: %s" % (self.path, name, e))

    def vector(self, name, width, n):
        try:
            return unpack_vector(self.member(name), width, int(n), name)
        except LegacyError as e:
            if str(e).startswith(str(self.path)):
                raise
            raise LegacyError("%s: %s" % (self.path, e))

    def close(self):
        self.z.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
        return False
