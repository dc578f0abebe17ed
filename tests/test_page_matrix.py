"""Type x encoding x page-layout matrix over hand-assembled pages (tests/pagekit.py).

Every other parity test decodes what pyarrow wrote; the contract is what parquet-mr 1.12.2 reads
(ParquetReader.java:139-177 over parquet-mr's column readers). Each cell here is one column chunk of
four pages (4,500 / 4,097 / 77 / 1 entries: across the 4,096-entry flat block, the 2,048- and
512-entry tiles, a partial last bit-packed group); the cells of one test id are the columns of one
file, so one decode call covers them all. Axes: physical type (FLBA at widths 1, 5, 16, 33), every
encoding the oracle's decode_values accepts for the type, five page layouts (pagekit.LAYOUTS),
REQUIRED / 30 % nulls / an all-null page next to an all-present one, and for dictionary cells the
id widths 0..32 with dictionaries of min(2^bw, 300) entries (so wide widths are non-minimal) in
three run styles. The expected arrays come from the inputs (by construction); the CPU test pins the
oracle (and pyarrow, where it opens the file) to them, the GPU test the HIP path, bit-exactly, and
the page-done flags prove which kernels saw which pages."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import pagekit as K
from conftest import GOLDEN
from golden_util import assert_chunk_equal

PAGE_SIZES = (4500, 4097, 77, 1)
ID_WIDTHS = (0, 1, 2, 7, 8, 9, 16, 17, 24, 31, 32)
DICT_TYPES = {"i32": (K.INT32, 0), "i64": (K.INT64, 0), "i96": (K.INT96, 0), "flba5": (K.FLBA, 5), "ba": (K.BYTE_ARRAY, 0)}
DONE_FIXED, DONE_FLAT, DONE_NULL, DONE_PAGE = 1, 2, 4, 8

# (name, ptype, type_length, encoding) of the non-sweep cells; "dict" = a 300-entry dictionary at id
# width 9, PLAIN_DICTIONARY / RLE_DICTIONARY alternating
PLAIN_CELLS = [
    ("bool_plain", K.BOOLEAN, 0, K.PLAIN), ("bool_rle", K.BOOLEAN, 0, K.RLE),
    ("i32_plain", K.INT32, 0, K.PLAIN), ("i32_dbp", K.INT32, 0, K.DELTA_BINARY_PACKED),
    ("i64_plain", K.INT64, 0, K.PLAIN), ("i64_dbp", K.INT64, 0, K.DELTA_BINARY_PACKED),
    ("i96_plain", K.INT96, 0, K.PLAIN),
    ("f32_plain", K.FLOAT, 0, K.PLAIN), ("f32_bss", K.FLOAT, 0, K.BYTE_STREAM_SPLIT), ("f32_dict", K.FLOAT, 0, "dict"),
    ("f64_plain", K.DOUBLE, 0, K.PLAIN), ("f64_bss", K.DOUBLE, 0, K.BYTE_STREAM_SPLIT), ("f64_dict", K.DOUBLE, 0, "dict"),
    ("ba_plain", K.BYTE_ARRAY, 0, K.PLAIN), ("ba_dlba", K.BYTE_ARRAY, 0, K.DELTA_LENGTH_BYTE_ARRAY),
    ("ba_dba", K.BYTE_ARRAY, 0, K.DELTA_BYTE_ARRAY),
] + [(f"flba{w}_{e}", K.FLBA, w, enc) for w in (1, 5, 16, 33)
     for e, enc in (("plain", K.PLAIN), ("dba", K.DELTA_BYTE_ARRAY), ("dict", "dict"))]
NULL_MODES = ("req", "opt", "nullpage")

FILE_IDS = [f"plain-{lay}-{nm}" for lay in K.LAYOUTS for nm in NULL_MODES] + \
           [f"dict-{lay}-{t}" for lay in K.LAYOUTS for t in DICT_TYPES] + \
           ["nested-a", "nested-b", "dbp-par"]
DAMAGED = {"plain": "f32_dict", "dict": "bw9_req", "nested": "flba5_dict"}   # the cell damaged per file kind

_FILES = {}          # file id -> dict(path, cells, info): generated once per session
STATS = {"cells": 0, "pyarrow_unreadable": [], "pyarrow_not_compared": 0}


# ---------------------------------------------------------------- data
def _rng(*key):
    """A generator seeded by the key's text (stable across processes, unlike hash())."""
    return np.random.default_rng(sum(ord(c) * (i + 7) for i, c in enumerate("/".join(map(str, key)))))


def _letters(rng, n):
    return (rng.integers(0, 26, n) + 97).astype(np.uint8).tobytes()


def _fixed(rng, ptype, tl, n, sortish=False):
    """n random values of a fixed-width type as uint8 [n, width]."""
    w = K.width_of(ptype, tl)
    if ptype == K.BOOLEAN:
        v = rng.integers(0, 2, n)
        k = 50
        while k < n:   # runs of equal values among the coin flips
            ln = int(rng.integers(8, 90))
            v[k:k + ln] = v[k]
            k += ln + int(rng.integers(1, 150))
        return v.astype(np.uint8).reshape(-1, 1)
    if ptype == K.INT96:   # nanos of day + Julian day around the epoch: a timestamp every reader accepts
        out = np.zeros((n, 12), np.uint8)
        out[:, :8] = rng.integers(0, 86400 * 10**9, n).astype("<i8").view(np.uint8).reshape(-1, 8)
        out[:, 8:] = rng.integers(2440588 - 20000, 2440588 + 20000, n).astype("<i4").view(np.uint8).reshape(-1, 4)
        return out
    if sortish:   # a small alphabet, sorted: neighbours share prefixes
        a = rng.integers(0, 3, (n, w)).astype(np.uint8) + 65
        return a[np.lexsort(a.T[::-1])] if n else a
    return rng.integers(0, 256, (n, w)).astype(np.uint8)


def _ints(rng, ptype, n, page):
    """INT32 / INT64 values for DELTA_BINARY_PACKED: small deltas, or the whole range (wrapping deltas)."""
    dt, bits = ("<i4", 32) if ptype == K.INT32 else ("<i8", 64)
    if page % 2 == 0:
        v = np.cumsum(rng.integers(-1000, 5000, n)).astype(dt)
    else:
        v = rng.integers(-2**(bits - 1), 2**(bits - 1), n, dtype=np.int64).astype(dt)
    return v.view(np.uint8).reshape(-1, bits // 8)


def _strings(rng, n, sortish=False, long_ok=True):
    """BYTE_ARRAY values: short words, empties, and (n large enough) values longer than 4 KiB."""
    if sortish:
        stems = [b"apple", b"applesauce", b"apply", b"band", b"bandana", b"", b"zebra" * 7]
        out = sorted(stems[int(k)] + str(int(x)).encode() for k, x in zip(rng.integers(0, len(stems), n), rng.integers(0, 50000, n)))
    else:
        lens = rng.integers(0, 21, n)
        lens[rng.random(n) < 0.1] = 0
        blob = _letters(rng, int(lens.sum()))
        ends = np.cumsum(lens)
        out = [blob[e - ln:e] for e, ln in zip(ends, lens)]
    if long_ok and n >= 40:
        base = _letters(rng, 5000)
        out[n // 2] = base                                   # > 4 KiB
        out[n // 2 + 1] = base[:4500] + b"tail"               # and a > 4 KiB prefix shared with it
    return out


def _ids(rng, n, dn):
    ids = rng.integers(0, dn, n)
    k = 300   # (the first entries stay random: the damage test overwrites packed ids there)
    while k < n:
        ln = int(rng.integers(8, 70))
        ids[k:k + ln] = ids[k]
        k += ln + int(rng.integers(1, 260))
    return ids


def _present(rng, n, mode, page):
    if mode == "req":
        return None
    if mode in ("nullpage", "nullpage_wb"):
        if page == 0:
            return np.ones(n, bool)
        if page == 1:
            return np.zeros(n, bool)
    p = rng.random(n) >= 0.3
    if n > 3000:   # runs of nulls and of values among them (RLE level runs)
        p[1000:1400] = False
        p[2000:2600] = True
    return p


def _take(vals, idx):
    return [vals[int(i)] for i in idx] if isinstance(vals, list) else vals[idx]


def _encode(ptype, enc, vals, page, rng, style):
    """Value section of `vals` (may be empty: a well-formed empty stream)."""
    if enc == K.PLAIN:
        return K.plain(ptype, vals)
    if enc == K.RLE:
        return K.rle_boolean(vals, style, rng)
    if enc == K.DELTA_BINARY_PACKED:
        dt, bits = ("<i4", 32) if ptype == K.INT32 else ("<i8", 64)
        return K.dbp(np.ascontiguousarray(vals).view(dt).ravel(), bits=bits)
    if enc == K.DELTA_LENGTH_BYTE_ARRAY:
        return K.delta_length(vals)
    if enc == K.DELTA_BYTE_ARRAY:
        return K.delta_byte_array(vals if ptype == K.BYTE_ARRAY else K.as_rows(vals))
    if enc == K.BYTE_STREAM_SPLIT:
        return K.byte_stream_split(vals)
    raise AssertionError(enc)


def _cell(name, ptype, tl, enc, mode, layout, compress, seed, bw=None):
    """One flat column chunk of PAGE_SIZES pages. enc "dict": dictionary of min(2^bw, 300) entries."""
    rng = _rng(seed, name, layout.name)
    ch = K.Chunk(name, ptype, tl, optional=mode != "req", layout=layout, compress=compress)
    is_dict = enc == "dict"
    if is_dict:
        bw = 9 if bw is None else bw
        dn = min(2**bw, 300)
        dvals = _strings(rng, dn, long_ok=dn >= 4) if ptype == K.BYTE_ARRAY else _fixed(rng, ptype, tl, dn)
        # parquet-mr's v1 writer: PLAIN_DICTIONARY on the dictionary and the data pages; v2: PLAIN + RLE_DICTIONARY
        old = (bw + (mode != "req")) % 2 == 0
        ch.set_dictionary(dvals, K.PLAIN_DICTIONARY if old else K.PLAIN)
        enc = K.PLAIN_DICTIONARY if old else K.RLE_DICTIONARY
    for page, n in enumerate(PAGE_SIZES):
        present = _present(rng, n, mode, page)
        nv = n if present is None else int(present.sum())
        style = K.STYLES[(page + (bw or 0) + len(name)) % 3]
        if is_dict:
            ids = _ids(rng, nv, dn)
            vals = _take(dvals, ids)
            if nv == 0:
                body = b"" if mode == "nullpage" else bytes([bw])
            else:
                body = K.dict_indices(ids, bw, style, rng)
        else:
            sortish = enc == K.DELTA_BYTE_ARRAY
            if ptype == K.BYTE_ARRAY:
                vals = _strings(rng, nv, sortish)
            elif enc == K.DELTA_BINARY_PACKED:
                vals = _ints(rng, ptype, nv, page)
            else:
                vals = _fixed(rng, ptype, tl, nv, sortish)
            body = _encode(ptype, enc, vals, page, rng, style)
        ch.add_page(enc, body, present=present, vals=vals, style=style, rng=rng)
    return ch


def _nested_structure(rng, target):
    """defs / reps of one page of `target` entries: lists null, empty, or of 1-4 elements with null ones."""
    defs, reps = [], []
    while len(defs) < target - 4:
        r = rng.random()
        if r < 0.1:
            defs.append(0); reps.append(0)
        elif r < 0.2:
            defs.append(1); reps.append(0)
        else:
            k = int(rng.integers(1, 5))
            defs += [2 if x < 0.15 else 3 for x in rng.random(k)]
            reps += [0] + [1] * (k - 1)
    while len(defs) < target:
        defs.append(int(rng.integers(0, 2))); reps.append(0)
    return np.array(defs, np.uint8), np.array(reps, np.uint8)


NESTED_LEAVES = [("i32_plain", K.INT32, 0, K.PLAIN), ("flba5_dict", K.FLBA, 5, "dict"),
                 ("ba_dlba", K.BYTE_ARRAY, 0, K.DELTA_LENGTH_BYTE_ARRAY), ("bool_rle", K.BOOLEAN, 0, K.RLE),
                 ("f64_bss", K.DOUBLE, 0, K.BYTE_STREAM_SPLIT), ("flba5_dba", K.FLBA, 5, K.DELTA_BYTE_ARRAY),
                 # dictionary leaves at the id widths 0, 17 (non-minimal) and 32: k_decode's and the segment kernels' id extraction
                 ("i64_dict_bw0", K.INT64, 0, "dict"), ("i32_dict_bw32", K.INT32, 0, "dict"),
                 ("ba_dict_bw0", K.BYTE_ARRAY, 0, "dict"), ("ba_dict_bw17", K.BYTE_ARRAY, 0, "dict"),
                 ("ba_dict_bw32", K.BYTE_ARRAY, 0, "dict")]


def _nested_cells(layout, compress):
    srng = _rng("nested-structure", layout.name)
    structure = [_nested_structure(srng, n) for n in PAGE_SIZES]
    cells = []
    for name, ptype, tl, enc in NESTED_LEAVES:
        rng = _rng("nested", name, layout.name)
        ch = K.Chunk(name, ptype, tl, nested=True, layout=layout, compress=compress)
        if enc == "dict":
            bw = int(name.split("_bw")[1]) if "_bw" in name else 9
            dn = min(2**bw, 300)
            dvals = _strings(rng, dn, long_ok=False) if ptype == K.BYTE_ARRAY else _fixed(rng, ptype, tl, dn)
            ch.set_dictionary(dvals, K.PLAIN)
        for page, (defs, reps) in enumerate(structure):
            nv = int((defs == 3).sum())
            style = K.STYLES[page % 3]
            if enc == "dict":
                ids = _ids(rng, nv, dn)
                vals, body, e = _take(dvals, ids), K.dict_indices(ids, bw, style, rng), K.RLE_DICTIONARY
            else:
                vals = _strings(rng, nv) if ptype == K.BYTE_ARRAY else _fixed(rng, ptype, tl, nv, enc == K.DELTA_BYTE_ARRAY)
                body, e = _encode(ptype, enc, vals, page, rng, style), enc
            ch.add_page(e, body, defs=defs, reps=reps, vals=vals, style=style, rng=rng)
        cells.append(ch)
    return cells, int(sum((r == 0).sum() for _d, r in structure))


def _dbp_par_cells():
    """One 20,000-entry page each (above DBP_PAR_MIN = 16,384, pf_internal.h): the block-parallel path."""
    rng = _rng("dbp-par")
    n = 20000
    full = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
    ext = np.tile(np.array([2**63 - 1, -2**63, 0, -1], np.int64), n // 4)
    cells = []
    for name, v in (("i64_full_range", full), ("i64_constant", np.full(n, 123456789012345, np.int64)), ("i64_extremes", ext)):
        ch = K.Chunk(name, K.INT64, layout=K.LAYOUTS["a"])
        ch.add_page(K.DELTA_BINARY_PACKED, K.dbp(v, bits=64), vals=v.astype("<i8").view(np.uint8).reshape(-1, 8))
        cells.append(ch)
    return cells, n


def _build(fid, oracle, tmpdir):
    kind, _, rest = fid.partition("-")
    compress = oracle.snappy_compress
    if kind == "plain":
        lay, mode = rest.split("-")
        cells = [_cell(name, pt, tl, enc, mode, K.LAYOUTS[lay], compress, fid) for name, pt, tl, enc in PLAIN_CELLS]
        rows = sum(PAGE_SIZES)
    elif kind == "dict":
        lay, t = rest.split("-")
        pt, tl = DICT_TYPES[t]
        cells = []
        for bw in ID_WIDTHS:
            modes = ("req", "opt") + (("nullpage", "nullpage_wb") if bw in (0, 9, 32) else ())
            cells += [_cell(f"bw{bw}_{m}", pt, tl, "dict", m, K.LAYOUTS[lay], compress, fid, bw=bw) for m in modes]
        rows = sum(PAGE_SIZES)
    elif kind == "nested":
        cells, rows = _nested_cells(K.LAYOUTS[rest], compress)
    else:
        cells, rows = _dbp_par_cells()
    data, info = K.build_file(cells, rows)
    path = os.path.join(tmpdir, fid + ".parquet")
    with open(path, "wb") as f:
        f.write(data)
    return {"path": path, "cells": cells, "info": info, "expected": [c.expected() for c in cells], "kind": kind}


@pytest.fixture(scope="session")
def matrix_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("page_matrix"))


@pytest.fixture
def matrix_file(oracle, matrix_dir):
    def get(fid):
        if fid not in _FILES:
            _FILES[fid] = _build(fid, oracle, matrix_dir)
        return _FILES[fid]
    return get


def _damaged_file(f, tmp_path):
    """The file with 80 bytes of the damaged cell's first data page's value section set to 0xFF.
    Returns (path, column index)."""
    col = next(i for i, c in enumerate(f["cells"]) if c.name == DAMAGED[f["kind"]])
    off, ln = f["info"][col]["values"][0]
    assert ln >= 240, ln
    data = bytearray(open(f["path"], "rb").read())
    lay = f["cells"][col].layout
    if not lay.v2 and lay.codec == K.SNAPPY:   # levels and values are one Snappy stream: the values are its tail
        off += ln - 240
    data[off + 40:off + 120] = b"\xff" * 80
    p = tmp_path / "damaged.parquet"
    p.write_bytes(bytes(data))
    return str(p), col


def _make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# ---------------------------------------------------------------- CPU: oracle (and pyarrow) vs construction
@pytest.mark.parametrize("fid", FILE_IDS)
def test_oracle_matrix(oracle, matrix_file, fid):
    import pyarrow.parquet as pq
    f = matrix_file(fid)
    n = 0
    with oracle.open(f["path"]) as of:
        assert of.num_columns == len(f["cells"])
        for c, (cell, exp) in enumerate(zip(f["cells"], f["expected"])):
            o = of.decode(0, c)
            assert o["status"] == 0, (fid, cell.name, o["error"])
            assert_chunk_equal(o, exp, f"{fid} {cell.name} [oracle vs construction]")
            n += 1
    assert n == len(f["cells"])
    STATS["cells"] += n
    mg = _make_golden()
    try:
        pf = pq.ParquetFile(f["path"])
    except Exception as e:   # (recorded, never silent: test_matrix_report prints the list)
        STATS["pyarrow_unreadable"].append((fid, "*", repr(e)[:200]))
        pf = None
    read = 0
    for c, (cell, exp) in enumerate(zip(f["cells"], f["expected"])):
        if pf is None:
            break
        if cell.layout.level_enc == K.BIT_PACKED and cell.max_def > 0:
            # Arrow's level decoder reads the deprecated BIT_PACKED encoding LSB-first; the format and
            # parquet-mr's ByteBitPackingValuesReader (the contract here) are MSB-first: not comparable
            STATS["pyarrow_not_compared"] += 1
            continue
        try:
            tbl = pf.read_row_group(0, columns=[cell.name])
        except Exception as e:
            STATS["pyarrow_unreadable"].append((fid, cell.name, repr(e)[:200]))
            continue
        pa_exp = mg.expected_for_column(tbl, pf.metadata, c)
        assert_chunk_equal(pa_exp, exp, f"{fid} {cell.name} [pyarrow vs construction]")
        read += 1
    print(f"{fid}: {n} cells match the oracle, pyarrow read {read} of them")


@pytest.mark.parametrize("fid", [f for f in FILE_IDS if f != "dbp-par"])
def test_oracle_damage(oracle, matrix_file, tmp_path, fid):
    f = matrix_file(fid)
    bad, col = _damaged_file(f, tmp_path)
    with oracle.open(bad) as of:
        assert of.decode(0, col)["status"] != 0, f"{fid}: damage in {f['cells'][col].name} not reported"


def test_matrix_report():
    """Cell count and the cells pyarrow could not read (run after the oracle tests of this module)."""
    print(f"page matrix: {STATS['cells']} cells compared with the oracle")
    print(f"not compared with pyarrow (BIT_PACKED levels, which Arrow reads LSB-first): {STATS['pyarrow_not_compared']} cells")
    print(f"pyarrow could not read {len(STATS['pyarrow_unreadable'])} cells:")
    for item in STATS["pyarrow_unreadable"]:
        print("   ", item)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def decoder():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _ints_per_page(decoder, fn, k):
    from pfloor import _native
    f = getattr(_native.lib(), fn)
    f.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
    n = f(decoder.h, None, 0)
    out = (C.c_int * (k * n))()
    assert f(decoder.h, out, n) == n
    return [tuple(out[k * i:k * i + k]) for i in range(n)]


def _page_flags(decoder, f):
    """Per cell: [(done, direct, dbp_ok, seg_ok)] of its data pages (the batch's page records are in
    chunk order, a chunk's dictionary page first)."""
    done = _ints_per_page(decoder, "pf_debug_page_done", 2)
    paths = _ints_per_page(decoder, "pf_debug_page_paths", 3)
    out, k = [], 0
    for cell in f["cells"]:
        k += 1 if cell.dict else 0
        out.append([(done[k + i][0],) + paths[k + i] for i in range(len(cell.pages))])
        k += len(cell.pages)
    assert k == len(done), (k, len(done))
    return out


def _check_paths(fid, f, flags):
    """Which kernel took which page, from the guards in pf_flat.hip, pf_flat_dstr.hip, pf_flat_null.hip / pf_plan.cpp."""
    kind = f["kind"]
    fixed_by_bw, null_by_bw = {}, {}
    for cell, pf_ in zip(f["cells"], flags):
        done = [p[0] for p in pf_]
        encs = cell.encodings
        label = f"{fid} {cell.name} done={done}"
        bit_packed_levels = cell.layout.level_enc == K.BIT_PACKED and cell.max_def > 0
        if bit_packed_levels or (cell.ptype == K.BOOLEAN and K.RLE in encs and "rle" in cell.name) or \
                encs & {K.BYTE_STREAM_SPLIT, K.DELTA_LENGTH_BYTE_ARRAY, K.DELTA_BYTE_ARRAY}:
            # BIT_PACKED levels: the flat kernels' s.def_rle / def_enc != 3 guards; the other encodings:
            # plan_routes sends them to k_decode first (decode_first) -> whole-page k_decode, no done flag
            assert all(d == 0 for d in done), label
        if kind == "dict" and cell.layout.level_enc == K.RLE:
            bw = int(cell.name[2:].split("_")[0])
            if cell.ptype != K.BYTE_ARRAY and cell.max_def == 0:
                fixed_by_bw[bw] = fixed_by_bw.get(bw, False) or any(d & DONE_FIXED for d in done)
            if cell.ptype in (K.INT32, K.INT64) and cell.name.endswith("_opt"):
                # (k_lvl tables exist for 4- and 8-byte types only: plan_routes grids 2 / 3, pf_plan.cpp)
                null_by_bw[bw] = null_by_bw.get(bw, False) or any(d & DONE_NULL for d in done)
            if cell.ptype == K.BYTE_ARRAY:
                assert any(d & DONE_FLAT for d in done), label
        if kind == "dbp-par":
            assert [p[2] for p in pf_] == [1], f"{label}: not the block-parallel path {pf_}"
    assert all(fixed_by_bw.values()), (fid, "no DONE_FIXED page at id widths", [b for b, v in fixed_by_bw.items() if not v])
    assert all(null_by_bw.values()), (fid, "no DONE_NULL page at id widths", [b for b, v in null_by_bw.items() if not v])
    if kind == "dict" and fid.split("-")[1] != "b":
        t = fid.split("-")[2]
        if t != "ba":
            assert sorted(fixed_by_bw) == sorted(ID_WIDTHS)
        if t in ("i32", "i64"):
            assert sorted(null_by_bw) == sorted(ID_WIDTHS)


def _compare_all(got, f, fid, tag, skip=None):
    n = 0
    for c, (cell, exp) in enumerate(zip(f["cells"], f["expected"])):
        if c == skip:
            continue
        g = got[(0, c)]
        assert g["status"] == 0, (fid, cell.name, tag, g["status"], got["_error"])
        assert_chunk_equal(g, exp, f"{fid} {cell.name} [{tag} vs construction]")
        n += 1
    return n


@pytest.mark.gpu
@pytest.mark.parametrize("fid", FILE_IDS)
def test_gpu_matrix(decoder, matrix_file, switches, fid):
    from pfloor.decoder import decode_file
    f = matrix_file(fid)
    got = decode_file(f["path"], decoder=decoder)
    flags = _page_flags(decoder, f)
    for c, cell in enumerate(f["cells"]):   # every page's flags first: a failing cell shows its path
        print(f"{fid} {cell.name}: status {got[(0, c)]['status']} (done, direct, dbp_ok, seg_ok) {flags[c]}")
    assert _compare_all(got, f, fid, "gpu") == len(f["cells"])
    assert got["_status"] == 0, got["_error"]
    _check_paths(fid, f, flags)
    if f["kind"] == "nested":   # once more with every nested page on the segment kernels
        from pfloor.decoder import GpuDecoder
        with switches(PF_NEST_SEG=256), GpuDecoder(0) as d:
            seg = decode_file(f["path"], decoder=d)
            seg_flags = _page_flags(d, f)
        assert _compare_all(seg, f, fid, "gpu PF_NEST_SEG=256") == len(f["cells"])
        for cell, pf_ in zip(f["cells"], seg_flags):
            print(f"{fid} {cell.name} PF_NEST_SEG=256: (done, direct, dbp_ok, seg_ok) {pf_}")
            # plan_chunk (pf_plan.cpp) gives segments to PLAIN fixed-width and dictionary leaves; k_nest_lvl
            # takes RLE levels only, so with BIT_PACKED levels (layout b) the pages are decoded whole
            if cell.layout.level_enc == K.RLE and ("dict" in cell.name or cell.name == "i32_plain"):
                assert [p[3] for p in pf_] == [1] * len(pf_), f"{fid} {cell.name}: not on the segment kernels {pf_}"


@pytest.mark.gpu
@pytest.mark.parametrize("fid", [f for f in FILE_IDS if f != "dbp-par"])
def test_gpu_damage(decoder, oracle, matrix_file, tmp_path, fid):
    """0xFF over 80 value bytes of one cell: that chunk is reported (as the oracle does,
    test_oracle_damage), every other chunk of the batch stays bit-exact, and the clean file decodes
    afterwards on the same decoder."""
    from pfloor.decoder import decode_file
    f = matrix_file(fid)
    bad, col = _damaged_file(f, tmp_path)
    with oracle.open(bad) as of:
        assert of.decode(0, col)["status"] != 0
    got = decode_file(bad, decoder=decoder)
    assert got[(0, col)]["status"] != 0, f"{fid}: damage in {f['cells'][col].name} not reported"
    assert _compare_all(got, f, fid, "gpu, next to the damaged chunk", skip=col) == len(f["cells"]) - 1
    clean = decode_file(f["path"], decoder=decoder)
    assert clean["_status"] == 0, clean["_error"]
    assert _compare_all(clean, f, fid, "gpu, after the damaged file") == len(f["cells"])
