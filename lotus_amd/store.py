"""On-disk side of the index directory (``lotus/vector_store/faiss_vs.py:27-41``).

The reference keeps two files per index: ``{dir}/vecs`` (a Python pickle of the embeddings, re-read IN FULL by every
``get_vectors_from_index`` and every ``ids``-branch search, ``faiss_vs.py:38-41,59``) and ``{dir}/index`` (faiss binary).
Both are still written, so a directory built here loads in stock LOTUS and vice versa.  On top of that:

* rows are served from a memory map, never from an unpickle: float32 embeddings are mapped in place inside
  ``{dir}/index`` (its code section IS the row-major matrix); other storage types (fp16, fp64) get a raw
  ``{dir}/rows.f16`` / ``rows.f64`` written next to it, described by ``{dir}/rows.json``;
* a rank that owns rows ``[lo, hi)`` touches only those pages (per-rank partial load);
* ``signature()`` = (size, mtime) of the files an index was loaded from, so a directory rewritten by another
  process is noticed instead of served stale; ``rows.json`` records size, mtime and a sampled content stamp of the two
  reference files it was written with: untouched files are accepted at once, a copied directory keeps its row store after
  ONE exact comparison with the faiss file, and a foreign rewrite - even of a few rows of the same shape - voids it.
"""
from __future__ import annotations

import json
import os
import pickle
import struct

import numpy as np

from . import faiss_io

RAW_VERSION = 1
_DTYPES = {"f16": np.float16, "f32": np.float32, "f64": np.float64}


def _dtype_tag(dt) -> str:
    for tag, t in _DTYPES.items():
        if np.dtype(dt) == np.dtype(t):
            return tag
    raise ValueError(f"unsupported storage dtype {dt}")


def write_dir(index_dir: str, embeddings, host: np.ndarray, metric: int, raw: bool = True) -> None:
    """Persist an index: the reference's two files + (``raw``) the mappable row store.  ``embeddings`` is what the caller
    handed to ``index()`` (pickled as is when it is an ndarray, exactly as ``faiss_vs.py:27-28``), ``host`` its 2-D host
    image."""
    os.makedirs(index_dir, exist_ok=True)
    meta_path = os.path.join(index_dir, "rows.json")
    if os.path.exists(meta_path):
        os.remove(meta_path)  # never leave a description of rows that are being replaced
    with open(os.path.join(index_dir, "vecs"), "wb") as fp:
        pickle.dump(embeddings if isinstance(embeddings, np.ndarray) else host, fp)
    faiss_io.write_index_flat(os.path.join(index_dir, "index"), host, metric)
    if not raw:
        return
    tag = _dtype_tag(host.dtype)
    meta = {"version": RAW_VERSION, "n": int(host.shape[0]), "d": int(host.shape[1]), "dtype": tag, "metric": int(metric),
            # the reference's two files as they are NOW: a writer that does not know about rows.json (stock LOTUS re-running
            # sem_index into this directory) changes them, and the description below is then void (_described_rows)
            "written_with": _file_stamps(index_dir)}
    if tag == "f32":
        meta["file"] = "index"  # mapped in place: the faiss file's code section is the float32 matrix
    else:
        meta["file"] = f"rows.{tag}"
        np.ascontiguousarray(host).tofile(os.path.join(index_dir, meta["file"]))
    tmp = meta_path + ".tmp"
    with open(tmp, "w") as fp:
        json.dump(meta, fp)
    os.replace(tmp, meta_path)  # the description appears only once the rows are complete


_STAMP_BLOCK = 4096
_STAMP_BLOCKS = 16


def _fingerprint(path: str, size: int) -> str:
    """Content stamp of a file that survives a copy: blake2b over its size and 16 evenly spaced 4 KB blocks (first and last
    included) - 64 KB read whatever the file's size.  A re-index with other embeddings changes the sampled rows; an mtime
    (round 3's stamp) changed with every `cp -r` / rsync and voided a perfectly good row store."""
    import hashlib

    h = hashlib.blake2b(digest_size=16)
    h.update(str(size).encode())
    with open(path, "rb") as fp:
        last = max(0, size - _STAMP_BLOCK)
        for i in range(_STAMP_BLOCKS):
            fp.seek(last * i // (_STAMP_BLOCKS - 1))
            h.update(fp.read(_STAMP_BLOCK))
    return h.hexdigest()


def _file_stamps(index_dir: str) -> dict:
    """[size, sampled fingerprint, mtime_ns] of the reference's two files."""
    out = {}
    for name in ("index", "vecs"):
        path = os.path.join(index_dir, name)
        try:
            st = os.stat(path)
            out[name] = [int(st.st_size), _fingerprint(path, int(st.st_size)), int(st.st_mtime_ns)]
        except FileNotFoundError:
            out[name] = [-1, "", -1]
    return out


def _row_store_matches_index(index_dir: str, meta: dict) -> bool:
    """EXACT check that ``rows.f16|f64`` still holds the embeddings ``{dir}/index`` was written from: the faiss file's code
    section is the float32 cast of the embeddings (``faiss_vs.py:24``), so the row store cast to float32 must equal it value
    for value.  One sequential pass over both files, only taken when the cheap (size, mtime) test could not decide."""
    codes = _mmap_flat_or_none(os.path.join(index_dir, "index"))
    n, d, tag = int(meta["n"]), int(meta["d"]), meta["dtype"]
    if codes is None or codes.shape != (n, d):
        return False
    path = os.path.join(index_dir, meta["file"])
    if not os.path.exists(path) or os.path.getsize(path) != n * d * np.dtype(_DTYPES[tag]).itemsize:
        return False
    if n == 0:
        return True
    rows = np.memmap(path, dtype=_DTYPES[tag], mode="r", shape=(n, d))
    step = max(1, (64 << 20) // (4 * d))
    for r0 in range(0, n, step):
        a = np.asarray(rows[r0:r0 + step]).astype(np.float32)
        if not np.array_equal(a.view(np.uint32), np.asarray(codes[r0:r0 + step]).view(np.uint32)):
            return False
    return True


def _stamps_still_valid(index_dir: str, meta: dict) -> bool:
    """Is the row store ``rows.json`` describes still the one the reference's two files were written with?

    * size of ``index`` / ``vecs`` changed                     -> no;
    * size and mtime both as recorded                          -> yes (nobody touched the files);
    * same size, other mtime (``cp -r`` / rsync / a re-index of the same shape by a writer that does not know rows.json):
      the sampled fingerprint must match - 64 KB of a file of gigabytes cannot rule out a rewrite of a few rows, so it only
      screens - and then the row store is compared with the faiss file's code section EXACTLY.  A float32 store is the faiss
      file itself (mapped in place): whatever it holds now is what a search must see, the fingerprint screen is enough.
    After a full comparison the new mtimes are recorded (best effort) so that the next open is cheap again."""
    stamps = meta.get("written_with")
    if stamps is None:
        return True
    now = _file_stamps(index_dir)
    same_time = True
    for name in ("index", "vecs"):
        was = list(stamps.get(name, [-2, ""]))
        if was[0] != now[name][0]:
            return False
        same_time &= len(was) >= 3 and was[2] == now[name][2]
    if same_time:
        return True
    if any(list(stamps[name])[1] != now[name][1] for name in ("index", "vecs")):
        return False
    if meta.get("file") == "index":
        return True
    if not _row_store_matches_index(index_dir, meta):
        return False
    try:
        meta = dict(meta, written_with=now)
        # several ranks may open the same copied directory at once: every writer gets a temporary file of its own, the rename
        # is atomic, the last one wins (they all write the same stamps)
        import tempfile

        fd, tmp = tempfile.mkstemp(prefix="rows.json.", suffix=".tmp", dir=index_dir)
        try:
            with os.fdopen(fd, "w") as fp:
                json.dump(meta, fp)
            os.replace(tmp, os.path.join(index_dir, "rows.json"))
        except OSError:
            try:
                os.unlink(tmp)
            except OSError:
                pass
    except OSError:
        pass
    return True


def _mmap_flat_or_none(path: str):
    """The code section of a faiss ``IndexFlat`` file as a memmap, or None when the file is something else -
    ``FaissVS(factory_string="IVF.." / "HNSW..")`` (``faiss_vs.py:14,23,30``) writes a non-flat index, whose rows can only
    come from the ``vecs`` pickle."""
    try:
        return faiss_io.mmap_index_flat(path)[0]
    except (ValueError, struct.error, OSError):
        return None


def signature(index_dir: str):
    sig = []
    for name in ("rows.json", "index", "vecs"):
        try:
            st = os.stat(os.path.join(index_dir, name))
            sig.append((name, st.st_size, st.st_mtime_ns))
        except FileNotFoundError:
            sig.append((name, -1, -1))
    return tuple(sig)


def _described_rows(index_dir: str):
    """The memmap ``rows.json`` describes, or None."""
    meta_path = os.path.join(index_dir, "rows.json")
    if not os.path.exists(meta_path):
        return None
    try:
        with open(meta_path) as fp:
            meta = json.load(fp)
        n, d, tag = int(meta["n"]), int(meta["d"]), meta["dtype"]
    except (OSError, ValueError, KeyError, TypeError):
        return None
    if meta.get("version") != RAW_VERSION or tag not in _DTYPES:
        return None
    if not _stamps_still_valid(index_dir, meta):
        return None  # `index` / `vecs` were rewritten by a writer that left this description (and rows.f16|f64) behind
    if meta["file"] == "index":
        rows = _mmap_flat_or_none(os.path.join(index_dir, "index"))
        return rows if (rows is not None and rows.shape == (n, d)) else None
    path = os.path.join(index_dir, meta["file"])
    if not os.path.exists(path) or os.path.getsize(path) != n * d * np.dtype(_DTYPES[tag]).itemsize:
        return None
    if n == 0:
        return np.zeros((0, d), _DTYPES[tag])
    return np.memmap(path, dtype=_DTYPES[tag], mode="r", shape=(n, d))


def open_stored_rows(index_dir: str):
    """-> (rows [n, d] in the STORED dtype, how).  What ``get_vectors_from_index`` serves (``faiss_vs.py:38-41``): a
    read-only memmap when the directory carries the row store ("raw" / "index-mmap"), else the unpickled ``vecs`` of a
    directory written by stock LOTUS ("pickle")."""
    rows = _described_rows(index_dir)
    if rows is not None:
        return rows, "mmap"
    with open(os.path.join(index_dir, "vecs"), "rb") as fp:
        return np.asarray(pickle.load(fp)), "pickle"


def open_device_rows(index_dir: str):
    """-> (rows [n, d], how) to build the device image from; always mappable: the row store when present, else the code
    section of ``{dir}/index`` - the float32 cast of the embeddings, i.e. exactly the values faiss itself searches
    (``faiss_vs.py:34,75``).  A rank slices ``rows[lo:hi]`` and reads only those pages; nothing is unpickled."""
    rows = _described_rows(index_dir)
    if rows is not None:
        return rows, "mmap"
    idx = os.path.join(index_dir, "index")
    if os.path.exists(idx):
        rows = _mmap_flat_or_none(idx)
        if rows is not None:
            return rows, "index-mmap"
    with open(os.path.join(index_dir, "vecs"), "rb") as fp:  # no mappable file: only the pickle has the rows
        return np.asarray(pickle.load(fp)), "pickle"


# ---- IVF sidecar --------------------------------------------------------------------------------------------------------
# An IVF store (HipVS(factory_string="IVF<nlist>,Flat")) writes the directory exactly as a flat one - stock LOTUS and
# FaissVS("Flat") still read it - plus ``{dir}/ivf.npz``: the trained centroids and the inverted lists (row numbers), so
# that a reload needs no k-means.  It is stamped with the content stamp of ``index`` / ``vecs`` (``_file_stamps``) and void
# once either file was rewritten.  Plain arrays only: it is read with ``allow_pickle=False``.
IVF_SIDECAR = "ivf.npz"
IVF_VERSION = 1


def _write_sidecar(index_dir: str, name: str, header: dict, arrays: dict) -> None:
    """Write ``{dir}/{name}`` atomically (temporary file + rename): the header, stamped with the content stamp of ``index`` /
    ``vecs`` as they are now, as a JSON string beside the arrays."""
    import tempfile

    header = dict(header, written_with=_file_stamps(index_dir))
    fd, tmp = tempfile.mkstemp(prefix=os.path.splitext(name)[0] + ".", suffix=".npz.tmp", dir=index_dir)
    try:
        with os.fdopen(fd, "wb") as fp:
            np.savez(fp, header=np.array(json.dumps(header)), **arrays)
        os.replace(tmp, os.path.join(index_dir, name))
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise


def _read_sidecar(index_dir: str, name: str, want: dict, keys: tuple):
    """-> (header, [the arrays ``keys``]) of ``{dir}/{name}``, or None when it is missing or unreadable, its header is not
    what ``want`` names, or ``index`` / ``vecs`` changed since it was written."""
    path = os.path.join(index_dir, name)
    if not os.path.exists(path):
        return None
    try:
        with np.load(path, allow_pickle=False) as z:
            header = json.loads(str(z["header"]))
            arrays = [np.array(z[key]) for key in keys]
    except (OSError, ValueError, KeyError, TypeError):
        return None
    if not isinstance(header, dict) or any(header.get(key) != val for key, val in want.items()):
        return None
    if not _ivf_stamps_valid(index_dir, header.get("written_with")):
        return None
    return header, arrays


def write_ivf(index_dir: str, nlist: int, metric: int, pack_mode: int, centroids: np.ndarray, offsets: np.ndarray,
              rows: np.ndarray) -> None:
    """Write the sidecar atomically (temporary file + rename)."""
    n, d = int(rows.shape[0]), int(centroids.shape[1])
    header = {"version": IVF_VERSION, "nlist": int(nlist), "metric": int(metric), "pack": int(pack_mode), "d": d, "n": n}
    _write_sidecar(index_dir, IVF_SIDECAR, header, {
        "centroids": np.ascontiguousarray(centroids, dtype=np.float32), "offsets": np.ascontiguousarray(offsets, dtype=np.int64),
        "rows": np.ascontiguousarray(rows, dtype=np.uint32)})


def _ivf_stamps_valid(index_dir: str, stamps) -> bool:
    """The sidecar's stamp is ``rows.json``'s (``_file_stamps``: size, sampled fingerprint and mtime of ``index`` / ``vecs``),
    but it is accepted only while ALL of it is unchanged.  ``_stamps_still_valid`` also keeps a row store whose files were
    copied (same size and fingerprint, new mtime) after an exact comparison with the faiss file; the lists have no such
    comparison - the sampled fingerprint alone cannot rule out a rewrite of a few rows - and retraining them costs one device
    k-means (a fraction of a second at 1 M rows), after which the rewritten sidecar carries the new mtimes."""
    if not isinstance(stamps, dict):
        return False
    now = _file_stamps(index_dir)
    for name in ("index", "vecs"):
        was = list(stamps.get(name, []))
        if len(was) < 3 or now[name][0] < 0 or was[:3] != list(now[name]):
            return False
    return True


def read_ivf(index_dir: str, nlist: int, metric: int, pack_mode: int, d: int, n: int):
    """-> (centroids float32 [nlist_eff, d], offsets int64 [nlist_eff + 1], rows uint32 [n]) from a valid sidecar written for
    this nlist, metric, pack mode and shape, else None (missing, unreadable, stale or built otherwise)."""
    want = {"version": IVF_VERSION, "nlist": int(nlist), "metric": int(metric), "pack": int(pack_mode), "d": int(d), "n": int(n)}
    side = _read_sidecar(index_dir, IVF_SIDECAR, want, ("centroids", "offsets", "rows"))
    if side is None:
        return None
    c, off, rows = side[1]
    m = int(c.shape[0]) if c.ndim == 2 else -1
    if (m < 1 or c.shape[1] != d or c.dtype != np.float32 or off.shape != (m + 1,) or off.dtype != np.int64
            or rows.shape != (n,) or rows.dtype != np.uint32 or off[0] != 0 or off[-1] > n or (np.diff(off) < 0).any()
            or (n and int(rows.max(initial=0)) >= n)):
        return None
    return c, off, rows


# ---- IVF-SQ8 sidecar ----------------------------------------------------------------------------------------------------
# An IVF-SQ8 store (HipVS(factory_string="IVF<nlist>,SQ8")) writes everything an IVF-Flat store writes - ``ivf.npz`` included,
# so an "IVF<nlist>,Flat" store of the same nlist reuses the lists - plus ``{dir}/ivf_sq8.npz``: the codec (vmin, vdiff, in
# the stored scale of the recorded pack exponent) and the codes and residual norms in list order.  It is stamped like
# ``ivf.npz`` and names the lists it was encoded against (``ivf_digest``), so it only counts together with that sidecar.
IVF_SQ8_SIDECAR = "ivf_sq8.npz"
IVF_SQ8_VERSION = 1


def ivf_digest(centroids: np.ndarray, offsets: np.ndarray, rows: np.ndarray) -> str:
    """Content digest of an IVF index's centroids and lists, as ``write_ivf`` stores them."""
    import hashlib

    h = hashlib.sha256()
    for a, dt in ((centroids, np.float32), (offsets, np.int64), (rows, np.uint32)):
        h.update(np.ascontiguousarray(a, dtype=dt).tobytes())
    return h.hexdigest()


def write_ivf_sq8(index_dir: str, nlist: int, metric: int, pack_mode: int, exp: int, vmin: np.ndarray, vdiff: np.ndarray,
                  codes: np.ndarray, rnorm: np.ndarray, lists_digest: str) -> None:
    """Write the SQ8 sidecar atomically (temporary file + rename)."""
    n, d = int(codes.shape[0]), int(codes.shape[1])
    header = {"version": IVF_SQ8_VERSION, "nlist": int(nlist), "metric": int(metric), "pack": int(pack_mode), "exp": int(exp),
              "d": d, "n": n, "lists": str(lists_digest)}
    _write_sidecar(index_dir, IVF_SQ8_SIDECAR, header, {
        "vmin": np.ascontiguousarray(vmin, dtype=np.float32), "vdiff": np.ascontiguousarray(vdiff, dtype=np.float32),
        "codes": np.ascontiguousarray(codes, dtype=np.uint8), "rnorm": np.ascontiguousarray(rnorm, dtype=np.float32)})


def read_ivf_sq8(index_dir: str, nlist: int, metric: int, pack_mode: int, exp: int, d: int, n: int, lists_digest: str):
    """-> (vmin float32 [d], vdiff float32 [d], codes uint8 [n, d] in list order, rnorm float32 [n]) from a valid SQ8 sidecar
    written for these lists (``ivf_digest``), nlist, metric, pack mode and exponent and shape, else None."""
    want = {"version": IVF_SQ8_VERSION, "nlist": int(nlist), "metric": int(metric), "pack": int(pack_mode), "exp": int(exp),
            "d": int(d), "n": int(n), "lists": str(lists_digest)}
    side = _read_sidecar(index_dir, IVF_SQ8_SIDECAR, want, ("vmin", "vdiff", "codes", "rnorm"))
    if side is None:
        return None
    vmin, vdiff, codes, rnorm = side[1]
    if (vmin.shape != (d,) or vdiff.shape != (d,) or vmin.dtype != np.float32 or vdiff.dtype != np.float32
            or codes.shape != (n, d) or codes.dtype != np.uint8 or rnorm.shape != (n,) or rnorm.dtype != np.float32):
        return None
    return vmin, vdiff, codes, rnorm


# ---- IVF-PQ sidecar -----------------------------------------------------------------------------------------------------
# An IVF-PQ store (HipVS(factory_string="IVF<nlist>,PQ<M>")) writes everything an IVF-Flat store writes - ``ivf.npz``
# included - plus ``{dir}/ivf_pq.npz``: the codebooks (in the stored scale of the recorded pack exponent) and the codes and
# beta terms in list order.  Like ``ivf_sq8.npz`` it is stamped and names the lists it was encoded against (``ivf_digest``).
IVF_PQ_SIDECAR = "ivf_pq.npz"
IVF_PQ_VERSION = 1


def write_ivf_pq(index_dir: str, nlist: int, metric: int, pack_mode: int, exp: int, codebooks: np.ndarray, codes: np.ndarray,
                 beta: np.ndarray, lists_digest: str) -> None:
    """Write the PQ sidecar atomically (temporary file + rename)."""
    M, ksub, dsub = (int(v) for v in codebooks.shape)
    header = {"version": IVF_PQ_VERSION, "nlist": int(nlist), "metric": int(metric), "pack": int(pack_mode), "exp": int(exp),
              "d": M * dsub, "M": M, "ksub": ksub, "n": int(codes.shape[0]), "lists": str(lists_digest)}
    _write_sidecar(index_dir, IVF_PQ_SIDECAR, header, {
        "codebooks": np.ascontiguousarray(codebooks, dtype=np.float32), "codes": np.ascontiguousarray(codes, dtype=np.uint8),
        "beta": np.ascontiguousarray(beta, dtype=np.float32)})


def read_ivf_pq(index_dir: str, nlist: int, metric: int, pack_mode: int, exp: int, d: int, M: int, n: int, lists_digest: str):
    """-> (codebooks float32 [M, ksub, d / M], codes uint8 [n, M] in list order, beta float32 [n]) from a valid PQ sidecar
    written for these lists (``ivf_digest``), nlist, metric, pack mode, exponent, M and shape, else None."""
    want = {"version": IVF_PQ_VERSION, "nlist": int(nlist), "metric": int(metric), "pack": int(pack_mode), "exp": int(exp),
            "d": int(d), "M": int(M), "n": int(n), "lists": str(lists_digest)}
    side = _read_sidecar(index_dir, IVF_PQ_SIDECAR, want, ("codebooks", "codes", "beta"))
    if side is None:
        return None
    ksub, (books, codes, beta) = side[0].get("ksub"), side[1]
    if (not isinstance(ksub, int) or not 1 <= ksub <= 256 or M < 1 or d % M != 0
            or books.shape != (M, ksub, d // M) or books.dtype != np.float32
            or codes.shape != (n, M) or codes.dtype != np.uint8 or beta.shape != (n,) or beta.dtype != np.float32
            or (n and int(codes.max(initial=0)) >= ksub)):
        return None
    return books, codes, beta
