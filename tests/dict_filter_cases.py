"""Cases and numpy reference of windows and predicates over kept dictionaries (pf_decode_row_group_dict_filter;
k_sel_dict / k_sel_mask_dict: csrc/pf_filter_dict.hip), assembled with tests/pagekit.py (TEST INFRASTRUCTURE ONLY).
tests/test_gpu_dict_filter.py decodes them; tests/test_dict_filter_cpu.py checks the reference against itself.

A batch is a file of chunks (dict_cases.Spec, or Plain: a chunk without a dictionary), optional windows and a list of
queries, each a conjunction [(chunk, op, lo, hi)] with Python values as bounds. The reference never uses the code under
test: filter_cases.eval_predicates over window_cases.slice_chunk of the expanded chunks gives the mask,
filter_cases.take_rows the expanded result, and a kept chunk's expected indices are the ids it was built from,
slot_ids[window][mask] (0 at nulls), next to the entries it was built from."""
import numpy as np

import dict_cases as DC
import filter_cases as FC
import pagekit as K
import window_cases as WC

SEL_TILE = 1024      # rows per workgroup round of the k_sel_* kernels (csrc/pf_internal.h)
FBLK = 4096          # entries per k_flat_ids block (csrc/pf_page_tables.h)
SELD_TILE = 256      # dictionary entries per k_sel_dict workgroup (csrc/pf_internal.h)
RANGE, IS_NULL, NOT_NULL = FC.RANGE, FC.IS_NULL, FC.NOT_NULL
DICT_SIZES = (0, 1, 63, 64, 65, 256, 257, SELD_TILE - 1, SELD_TILE, SELD_TILE + 1, 65536, 65537)
_NP = {K.INT32: np.int32, K.INT64: np.int64, K.FLOAT: np.float32, K.DOUBLE: np.float64}


def typed(ptype, values):
    """Python / numpy values as dictionary entries: uint8 [n, width]."""
    a = np.asarray(values, _NP[ptype])
    return a.view(np.uint8).reshape(len(a), a.dtype.itemsize)


def bound_bytes(ptype, v):
    """A bound's PLAIN bytes, as pf_predicate takes them."""
    if v is None:
        return None
    return bytes(v) if ptype == K.BYTE_ARRAY else _NP[ptype](v).tobytes()


class Plain:
    """A chunk without a dictionary: PLAIN pages, never kept."""

    def __init__(self, name, ptype, vals, present=None, compress=None, page=3000):
        self.ptype, self.kept, self.keep, self.eligible, self.n_dict = ptype, False, True, False, 0
        self.chunk = K.Chunk(name, ptype, optional=present is not None, compress=compress)
        n = len(present) if present is not None else len(vals)
        at = 0
        for a in range(0, max(n, 1), page):
            pr = None if present is None else np.asarray(present[a:a + page], bool)
            k = int(pr.sum()) if pr is not None else min(page, n - a)
            v = vals[at:at + k]
            at += k
            self.chunk.add_page(K.PLAIN, K.plain(ptype, v), present=pr, vals=v)


NULLS = {
    "none": lambda n: None,
    "every7th": lambda n: np.arange(n) % 7 != 6,
    "runs": lambda n: (np.arange(n) // 50) % 3 != 1,          # runs of 50 nulls: they cross the 64-row words
    "all": lambda n: np.zeros(n, bool),
}


def fill(spec, n, rng, nulls="none", pages=None, style="mr", level_style="mr"):
    """n rows into spec, split into pages; every entry of a small dictionary is used, the first and the last id of any."""
    present = NULLS[nulls](n)
    if spec.optional and present is None:
        present = np.ones(n, bool)
    nv = int(present.sum()) if present is not None else n
    ids = rng.integers(0, max(spec.n_dict, 1), nv)
    if nv and spec.n_dict:
        k = min(nv, spec.n_dict, 300)
        ids[:k] = np.arange(k)
        ids[-1] = spec.n_dict - 1
    a = va = 0
    for p, size in enumerate(pages or (n,)):
        pr = None if present is None else present[a:a + size]
        k = int(pr.sum()) if pr is not None else size
        spec.page(ids[va:va + k], present=pr, style=style, level_style=level_style, seed=p)
        a += size
        va += k
    assert a == n
    return spec


def canon(spec, e):
    """An expanded chunk (the oracle's arrays, or pagekit's expectation) with every count the reference reads."""
    out = {k: v for k, v in e.items() if k in WC.ARRAYS or k in WC.COUNTS}
    out.setdefault("num_rows", out["num_entries"])
    out["width"] = 0 if spec.ptype == K.BYTE_ARRAY else spec.chunk.width
    out["num_chars"] = int(len(out["chars"])) if "chars" in out else 0
    return out


def reference(specs, exp, windows, preds):
    """exp: the expanded chunks (canon). Returns (rows_in, selected row numbers or None without predicates, per chunk
    the expanded result, per chunk the kept result or None): a window that does not fit its chunk gives None for both."""
    win = []
    for c, e in enumerate(exp):
        skip, take = windows[c] if windows else (0, -1)
        rows = int(e["num_rows"])
        ok = 0 <= skip <= rows and (take < 0 or skip + take <= rows)
        win.append(WC.slice_chunk(e, skip, take) if ok else None)
    idx, rows_in = None, None
    if preds:
        cols = [(w, s.ptype) for w, s in zip(win, specs)]
        first = preds[0][0]
        rows_in = int(win[first]["num_rows"])
        mask = FC.eval_predicates([cols[first]] + cols, [(c + 1, op, lo, hi) for c, op, lo, hi in preds])
        idx = np.flatnonzero(mask)
    expanded, kept = [], []
    for c, (s, w) in enumerate(zip(specs, win)):
        if w is None:
            expanded.append(None)
            kept.append(None)
            continue
        r = FC.take_rows(w, idx) if idx is not None else w
        expanded.append(r)
        if not s.kept:
            kept.append(None)
            continue
        skip, take = windows[c] if windows else (0, -1)
        ids = s.expected_indices()
        ids = ids[skip:] if take < 0 else ids[skip:skip + take]
        if idx is not None:
            ids = ids[idx]
        k = {key: r[key] for key in ("num_entries", "num_slots", "num_values", "num_rows")}
        k.update(indices=ids, width=DC.index_width(s.n_dict), num_chars=0, dictionary=s.expected_dictionary())
        if "validity" in r:
            k["validity"] = r["validity"]
        kept.append(k)
    return rows_in, idx, expanded, kept


def materialized(kept, ptype):
    """numpy expansion of a kept expectation (not pfloor.decoder.materialize: the reference stands alone)."""
    ids = np.asarray(kept["indices"], np.int64)
    n = len(ids)
    valid = WC._bits(kept["validity"], n).astype(bool) if "validity" in kept else np.ones(n, bool)
    d = kept["dictionary"]
    out = {k: kept[k] for k in ("num_entries", "num_slots", "num_values", "num_rows")}
    if "validity" in kept:
        out["validity"] = kept["validity"]
    if ptype == K.BYTE_ARRAY:
        off = np.asarray(d["offsets"], np.int64)
        ch = np.asarray(d["chars"], np.uint8).tobytes()
        vals = [ch[off[i]:off[i + 1]] if v else b"" for i, v in zip(ids, valid)]
        no = np.zeros(n + 1, np.int32)
        np.cumsum([len(x) for x in vals], out=no[1:])
        out.update(offsets=no, chars=np.frombuffer(b"".join(vals), np.uint8), num_chars=int(no[-1]), width=0)
    else:
        w = int(d["width"])
        v = np.zeros((n, w), np.uint8)
        if valid.any():
            v[valid] = np.asarray(d["values"], np.uint8).reshape(-1, w)[ids[valid]]
        out.update(values=v.ravel(), num_chars=0, width=w)
    return out


class Batch:
    def __init__(self, name, build):
        self.name, self.build = name, build   # build(compress) -> (specs, windows or None, [(label, preds)])


def _mid(spec):
    """A bound that splits the dictionary's entries about in half (None for an empty dictionary)."""
    if not spec.n_dict:
        return None
    if spec.ptype == K.BYTE_ARRAY:
        return sorted(spec.dvals)[spec.n_dict // 2]
    v = np.sort(np.ascontiguousarray(spec.dvals).view(_NP[spec.ptype]).ravel())
    return v[spec.n_dict // 2].item()


def _entries(ptype, n, rng):
    if ptype == K.BYTE_ARRAY:
        return [b"k%05d" % ((i * 7919) % 100003) for i in range(n)]
    if ptype in (K.INT32, K.INT64):
        return typed(ptype, rng.permutation(n) - n // 2)
    return typed(ptype, (rng.permutation(n) - n // 2) / 4.0)


def _batches():
    out = []

    # ---- dictionary sizes (index widths 1, 2, 4; the bitmap's word and k_sel_dict's tile edges) x rows at the edges of
    # SEL_TILE and FBLK, as predicate chunks: a bound in the middle, one no entry matches, one every entry matches
    for rows, sizes in ((SEL_TILE - 1, (1, 63)), (SEL_TILE, (64, 65)), (SEL_TILE + 1, (255, 256, 257)), (FBLK - 1, (0, 65536)),
                        (FBLK, (65537,)), (FBLK + 1, (256, 300)), (3 * SEL_TILE, (257, 1))):
        def build(compress, rows=rows, sizes=sizes):
            rng = np.random.default_rng(rows)
            specs, qs = [], []
            for nd in sizes:
                for ptype, tname in ((K.INT32, "int32"), (K.BYTE_ARRAY, "binary")):
                    if nd > 300 and ptype == K.BYTE_ARRAY:
                        continue
                    opt = nd == 0 or (nd + ptype) % 2 == 0
                    s = DC.Spec(f"{tname}_{nd}", tname, _entries(ptype, nd, rng), optional=opt, compress=compress)
                    fill(s, rows, rng, nulls="all" if nd == 0 else ("every7th" if opt else "none"),
                         pages=(rows,) if rows < 3000 else (1500, rows - 1500))
                    c = len(specs)
                    specs.append(s)
                    m = _mid(s)
                    far = b"\xff\xff" if ptype == K.BYTE_ARRAY else 2 ** 31 - 1
                    qs += [(f"{s.chunk.name} <= mid", [(c, RANGE, None, m)]), (f"{s.chunk.name} >= mid", [(c, RANGE, m, None)]),
                           (f"{s.chunk.name} none", [(c, RANGE, far, None)]), (f"{s.chunk.name} all", [(c, RANGE, None, far)])]
                    if opt:
                        qs.append((f"{s.chunk.name} is null", [(c, IS_NULL, None, None)]))
            return specs, None, qs
        out.append(Batch(f"sizes-rows{rows}", build))

    # ---- every RANGE-able type, REQUIRED and OPTIONAL, with the values comparisons get wrong
    def types(compress):
        rng = np.random.default_rng(7)
        nan2 = np.array([0x7fc00001], np.uint32).view(np.float32)[0]
        dnan2 = np.array([0x7ff8000000000001], np.uint64).view(np.float64)[0]
        inf = float("inf")
        dicts = {
            "int32": typed(K.INT32, [-2 ** 31, -1, 0, 1, 2 ** 31 - 1, 7, -7]),
            "int64": typed(K.INT64, [-2 ** 63, -1, 0, 1, 2 ** 63 - 1, 2 ** 31, -2 ** 31 - 1]),
            "float": typed(K.FLOAT, [np.nan, nan2, -0.0, 0.0, inf, -inf, 1.5, -1.5, 3.4e38]),
            "double": typed(K.DOUBLE, [np.nan, dnan2, -0.0, 0.0, inf, -inf, 1.5, -1.5, 1e308]),
            "binary": [b"", b"a", b"ab", b"abc", b"ab", b"\xff", b"\x00", b"ab\x00", b"b" * 32, b"b" * 33, b"c" * 64, b"c" * 65,
                       b"d" * 300, b"e" * 5000, b"e" * 4096, b"e" * 4095, b"e" * 4097],
        }
        bounds = {
            "int32": [(-2 ** 31, None), (None, 2 ** 31 - 1), (2 ** 31 - 1, None), (None, -2 ** 31), (0, 0), (-1, 1), (8, None)],
            "int64": [(-2 ** 63, None), (None, 2 ** 63 - 1), (2 ** 63 - 1, None), (None, -2 ** 63), (0, 0), (-2 ** 31 - 1, 2 ** 31)],
            "float": [(np.nan, None), (None, np.nan), (-0.0, 0.0), (0.0, None), (None, -0.0), (-inf, inf), (inf, None), (None, -inf),
                      (None, None), (1.5, 1.5)],
            "double": [(np.nan, None), (None, np.nan), (-0.0, 0.0), (0.0, None), (None, -0.0), (-inf, inf), (inf, None),
                       (None, -inf), (None, None), (-1.5, 1.5)],
            "binary": [(b"", b""), (b"ab", b"ab"), (b"ab", None), (None, b"ab"), (b"abc", b"abd"), (b"e" * 4096, b"e" * 4096),
                       (b"e" * 4096, None), (None, b"e" * 4096), (b"b" * 33, b"c" * 64), (b"\xff", None), (None, b"\x00"), (None, None)],
        }
        n = 2 * SEL_TILE + 77
        specs, qs = [], []
        for tname, dv in dicts.items():
            for opt in (False, True):
                s = DC.Spec(f"{tname}_{int(opt)}", tname, dv, optional=opt, compress=compress)
                fill(s, n, rng, nulls="runs" if opt else "none", pages=(900, n - 900))
                c = len(specs)
                specs.append(s)
                for lo, hi in bounds[tname]:
                    qs.append((f"{s.chunk.name} in [{str(lo)[:12]}, {str(hi)[:12]}]", [(c, RANGE, lo, hi)]))
                if opt:
                    qs += [(f"{s.chunk.name} not null", [(c, NOT_NULL, None, None)])]
        return specs, None, qs
    out.append(Batch("types", types))

    # ---- rows_selected at every residue the gather's 16-byte groups have, over payloads of index widths 1, 2 and 4:
    # an expanded predicate chunk whose values are a permutation of the row numbers selects exactly k scattered rows
    def residues(compress):
        rng = np.random.default_rng(11)
        n = FBLK + 1
        perm = (np.arange(n, dtype=np.int64) * 7919) % n
        specs = [Plain("rownum", K.INT32, typed(K.INT32, perm), compress=compress)]
        for nd, tname, opt in ((25, "binary", True), (300, "int64", False), (65537, "int32", True), (200, "flba5", False)):
            dv = _entries(DC.TYPES[tname][0], nd, rng) if tname != "flba5" else DC.make_dict(tname, nd, rng)
            s = DC.Spec(f"pay_{nd}", tname, dv, optional=opt, compress=compress)
            specs.append(fill(s, n, rng, nulls="every7th" if opt else "none", pages=(33, 4000, n - 4033)))
        ks = list(range(0, 34)) + [63, 64, 65, 127, 128, 129, SEL_TILE - 1, SEL_TILE, SEL_TILE + 1, n]
        return specs, None, [(f"{k} rows", [(0, RANGE, None, k - 1)]) for k in ks]
    out.append(Batch("selected-residues", residues))

    # ---- null shapes, INT96 and FIXED_LEN_BYTE_ARRAY kept chunks as payloads and under IS_NULL / NOT_NULL
    def nulls(compress):
        rng = np.random.default_rng(13)
        n = SEL_TILE + 300
        specs, qs = [], []
        for tname, nd, shape in (("int32", 9, "none"), ("int64", 9, "every7th"), ("binary", 9, "runs"), ("double", 9, "all"),
                                 ("int32", 0, "all"), ("binary", 0, "all"), ("int96", 5, "runs"), ("flba5", 300, "every7th"),
                                 ("flba16", 3, "none")):
            pt = DC.TYPES[tname][0]
            dv = _entries(pt, nd, rng) if pt in _NP or pt == K.BYTE_ARRAY else DC.make_dict(tname, nd, rng)
            s = DC.Spec(f"{tname}_{nd}_{shape}", tname, dv, optional=True, compress=compress)
            c = len(specs)
            specs.append(fill(s, n, rng, nulls=shape))
            qs += [(f"{s.chunk.name} is null", [(c, IS_NULL, None, None)]), (f"{s.chunk.name} not null", [(c, NOT_NULL, None, None)])]
            if pt in _NP or pt == K.BYTE_ARRAY:
                qs.append((f"{s.chunk.name} any value", [(c, RANGE, None, None)]))
                qs.append((f"{s.chunk.name} >= mid", [(c, RANGE, _mid(s), None)]))
        return specs, None, qs
    out.append(Batch("nulls-int96-flba", nulls))

    # ---- conjunctions: kept and expanded predicate chunks mixed, two predicates on one kept chunk, an asked-for chunk
    # that fell back to PLAIN beside kept ones, a page that takes k_flat_ids' slow path
    def conj(compress):
        rng = np.random.default_rng(17)
        n = 2 * SEL_TILE + 5
        a = fill(DC.Spec("a", "int32", typed(K.INT32, np.arange(40) - 20), compress=compress), n, rng, pages=(1000, n - 1000))
        b = fill(DC.Spec("b", "binary", [b"s%02d" % i for i in range(90)], optional=True, compress=compress), n, rng, nulls="every7th")
        c = fill(DC.Spec("c", "double", typed(K.DOUBLE, np.arange(400) / 8.0), compress=compress), n, rng, style="mixed")
        assert c.paths[-1][0] == "slow"
        d = DC.Spec("d", "int64", typed(K.INT64, np.arange(30)), compress=compress)
        fill(d, n - 300, rng)
        d.plain_page(300, rng)                                      # asked for, not eligible: filtered expanded
        e = Plain("e", K.INT32, typed(K.INT32, rng.integers(0, 100, n)), compress=compress)
        f = fill(DC.Spec("f", "flba16", DC.make_dict("flba16", 70, rng), optional=True, compress=compress), n, rng, nulls="runs")
        specs = [a, b, c, d, e, f]
        p = {"a": (0, RANGE, -10, 10), "a2": (0, RANGE, 0, None), "b": (1, RANGE, b"s10", b"s80"), "bn": (1, NOT_NULL, None, None),
             "c": (2, RANGE, 5.0, 40.0), "d": (3, RANGE, 3, 25), "e": (4, RANGE, 10, 90), "fn": (5, NOT_NULL, None, None)}
        qs = [("kept + kept", [p["a"], p["b"]]), ("kept + expanded", [p["a"], p["e"]]), ("expanded first", [p["e"], p["c"]]),
              ("two on one kept chunk", [p["a"], p["a2"]]), ("three", [p["b"], p["c"], p["d"]]),
              ("eight", [p["a"], p["a2"], p["b"], p["bn"], p["c"], p["d"], p["e"], p["fn"]]), ("ineligible only", [p["d"]])]
        return specs, None, qs
    out.append(Batch("conjunctions", conj))

    # ---- windows without predicates: skip and take at every residue mod 8 around a page edge, index widths 1, 2, 4
    edge = 1000
    wins = [(edge - 4 + r, 41) for r in range(8)] + [(edge - 3, 40 + r) for r in range(8)] + [(0, -1), (5, 0), (0, 2500), (2499, 1),
                                                                                               (17, -1), (2400, 200)]
    for k, (skip, take) in enumerate(wins):
        def windows(compress, skip=skip, take=take):
            rng = np.random.default_rng(19)
            n = 2500
            specs = []
            for nd, tname, opt in ((7, "binary", True), (300, "int32", True), (65537, "int64", False), (50, "flba5", True)):
                dv = _entries(DC.TYPES[tname][0], nd, rng) if tname != "flba5" else DC.make_dict(tname, nd, rng)
                s = DC.Spec(f"w_{nd}", tname, dv, optional=opt, compress=compress)
                specs.append(fill(s, n, rng, nulls="runs" if opt else "none", pages=(edge, n - edge)))
            specs.append(Plain("plain", K.INT64, typed(K.INT64, np.arange(n)), compress=compress))
            wl = [(skip, take)] * len(specs)
            if skip + take > n:   # past the rows of chunk 0 only: PF_ERR_INVALID_ARG on that chunk, the others stand
                wl = [(skip, take)] + [(skip, n - skip)] * (len(specs) - 1)
            return specs, wl, [("window", [])]
        out.append(Batch(f"window-{k}-skip{skip}-take{take}", windows))

    # ---- windows with predicates: a windowed chunk (moved into the twins, filtered back into the decode arena) beside
    # chunks of the window's length without one (filtered into the twins)
    def both(compress):
        rng = np.random.default_rng(23)
        n, skip = SEL_TILE + 90, 37
        big = fill(DC.Spec("moved", "binary", [b"m%03d" % i for i in range(300)], optional=True, compress=compress), n + skip + 11, rng,
                   nulls="every7th", pages=(500, n + skip + 11 - 500))
        big4 = fill(DC.Spec("moved4", "int32", _entries(K.INT32, 65537, rng), compress=compress), n + skip + 11, rng)
        stay = fill(DC.Spec("stays", "int64", typed(K.INT64, np.arange(20)), compress=compress), n, rng)
        exp = Plain("expanded", K.INT32, typed(K.INT32, rng.integers(0, 50, n)), compress=compress)
        specs = [big, big4, stay, exp]
        wins = [(skip, n), (skip, n), (0, -1), (0, -1)]
        qs = [("moved", [(0, RANGE, b"m100", b"m250")]), ("stays", [(2, RANGE, 5, 12)]), ("moved4", [(1, RANGE, 0, None)]),
              ("both", [(0, RANGE, b"m100", None), (2, RANGE, None, 15), (3, RANGE, 10, None)]), ("none", [(2, RANGE, 99, None)])]
        return specs, wins, qs
    out.append(Batch("windows-and-predicates", both))
    return out


BATCHES = {b.name: b for b in _batches()}
