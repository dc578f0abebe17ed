"""Cases of the kept-dictionary decode (pf_decode_row_group_dict, k_flat_ids / k_dict_pack: pf_flat_ids.hip), assembled
with tests/pagekit.py (TEST INFRASTRUCTURE ONLY). tests/test_gpu_dict_keep.py decodes them.

A case is a file of chunks. Every chunk remembers what it was built from: the dictionary's entries, the id of every slot
(0 at a null slot), whether the rule of include/pfloor.h keeps it, and per data page which path of k_flat_ids the
stated rule sends it down:
  slow  the id stream has more than RUN_CAP runs, or the page has entries that are not present (as k_runs sees it: its
        levels are not RLE runs of max_def only) and no usable level table -- none was planned (a v2 header with
        num_nulls = 0), the levels are BIT_PACKED, or they have more runs than lvl_table_cap(entries);
  fast  every other page, one count per FBLK block.
The run counts are read from the very streams the pages hold (count_runs), not assumed."""
import numpy as np

import pagekit as K

FBLK = 4096
RUN_CAP = 256
COUNTS = (1, 15, 16, 17, 4095, 4096, 4097, 2 * 4096 + 1)
V1S = K.Layout("v1s", False, K.SNAPPY)

# name -> (physical type, type_length)
TYPES = {"int32": (K.INT32, 0), "int64": (K.INT64, 0), "int96": (K.INT96, 0), "float": (K.FLOAT, 0), "double": (K.DOUBLE, 0),
         "flba5": (K.FLBA, 5), "flba16": (K.FLBA, 16), "binary": (K.BYTE_ARRAY, 0)}


def bw_of(n):
    return max(n - 1, 0).bit_length()


def index_width(n):
    return 1 if n <= 256 else (2 if n <= 65536 else 4)


def make_dict(tname, n, rng, strings="mixed"):
    """n dictionary entries: a uint8 array [n, width], or a list of bytes (strings: "mixed" has the empty string and a
    33-byte value among lengths 0 to 24; "short" is 1 to 6 bytes)."""
    ptype, tl = TYPES[tname]
    if ptype == K.BYTE_ARRAY:
        if strings == "short":
            return [bytes([97 + (i + k) % 26 for k in range(1 + i % 6)]) + b"%d" % i for i in range(n)]
        out = [bytes([65 + (i + k) % 26 for k in range(i % 25)]) for i in range(n)]
        if n > 3:
            out[3] = b"q" * 33
        return out
    return rng.integers(0, 256, (n, K.width_of(ptype, tl))).astype(np.uint8)


def count_runs(stream, bw, n_values):
    """Non-empty runs of a hybrid stream up to n_values values (what k_runs / k_lvl count), and whether all are RLE."""
    pos = covered = runs = 0
    all_rle, values = True, []
    while covered < n_values and pos < len(stream):
        h = shift = 0
        while True:
            b = stream[pos]
            pos += 1
            h |= (b & 0x7f) << shift
            shift += 7
            if not b & 0x80:
                break
        if h & 1:
            cnt = (h >> 1) * 8
            pos += (h >> 1) * bw
            all_rle = all_rle and cnt == 0
        else:
            cnt = h >> 1
            nb = (bw + 7) // 8
            if cnt:
                values.append(int.from_bytes(stream[pos:pos + nb], "little"))
            pos += nb
        if cnt:
            runs += 1
            covered += cnt
    return runs, all_rle, values


class Spec:
    """One chunk of a case and what it was built from."""

    def __init__(self, name, tname, dvals, optional=False, layout=K.LAYOUTS["a"], compress=None, dict_encoding=K.PLAIN):
        ptype, tl = TYPES[tname]
        self.tname, self.ptype, self.dvals, self.optional, self.layout = tname, ptype, dvals, optional, layout
        self.chunk = K.Chunk(name, ptype, type_length=tl, optional=optional, layout=layout, compress=compress)
        self.chunk.set_dictionary(dvals, encoding=dict_encoding)
        self.n_dict = len(dvals)
        self.slot_ids = []          # per page: the id of every slot, 0 at a null slot
        self.paths = []             # per page: ("fast", blocks) or ("slow", 1)
        self.eligible = True
        self.keep = True            # the flag the test passes for this chunk

    def values_of(self, ids):
        if self.ptype == K.BYTE_ARRAY:
            return [self.dvals[min(int(i), self.n_dict - 1)] for i in ids]
        return self.dvals[np.minimum(np.asarray(ids, np.int64), self.n_dict - 1)] if self.n_dict else self.dvals[:0]

    def page(self, ids, bw=None, style="mr", present=None, stream=None, encoding=K.RLE_DICTIONARY, level_style="mr", seed=0):
        """One dictionary data page: ids of the present values; present: bool per entry (OPTIONAL)."""
        ids = np.asarray(ids, np.uint64)
        bw = bw_of(self.n_dict) if bw is None else bw
        if stream is None:
            stream = K.hybrid(ids, bw, style, np.random.default_rng(seed + 1))
        n = len(present) if present is not None else len(ids)
        if self.optional and present is None:
            present = np.ones(n, bool)
        self.chunk.add_page(encoding, bytes([bw]) + stream, present=present, vals=self.values_of(ids), style=level_style,
                            rng=np.random.default_rng(seed + 2))
        slot = np.zeros(n, np.int64)
        if present is not None:
            slot[np.asarray(present, bool)] = ids.astype(np.int64)
        else:
            slot[:] = ids.astype(np.int64)
        self.slot_ids.append(slot)
        # which path (the rule in the module docstring)
        id_runs, _, _ = count_runs(stream, bw, len(ids))
        slow = n == 0 or id_runs > RUN_CAP
        if not slow and self.optional:
            nulls = int(n - np.asarray(present, bool).sum())
            if self.layout.level_enc == K.BIT_PACKED and not self.layout.v2:
                all_present, lvl_runs = False, None
            else:
                lv = K.hybrid(np.asarray(present, np.uint8), 1, level_style, np.random.default_rng(seed + 2))
                lvl_runs, all_rle, vals = count_runs(lv, 1, n)
                all_present = all_rle and all(v == 1 for v in vals)
            if not all_present:
                has_table = (not self.layout.v2) or nulls > 0      # v1 pages here carry no statistics: num_nulls = -1
                slow = not has_table or lvl_runs is None or lvl_runs > n // 8 + 64
        self.paths.append(("slow", 1) if slow else ("fast", max(1, (n + FBLK - 1) // FBLK)))

    def plain_page(self, n, rng):
        """A PLAIN page (the writer fell back): the chunk is no longer eligible."""
        ids = rng.integers(0, self.n_dict, n)
        vals = self.values_of(ids)
        self.chunk.add_page(K.PLAIN, K.plain(self.ptype, vals), present=np.ones(n, bool) if self.optional else None, vals=vals)
        self.eligible = False

    @property
    def kept(self):
        return self.eligible and self.keep

    def expected_indices(self):
        return np.concatenate(self.slot_ids) if self.slot_ids else np.zeros(0, np.int64)

    def expected_dictionary(self):
        """The dictionary as fetch returns it."""
        if self.ptype == K.BYTE_ARRAY:
            offs = np.zeros(self.n_dict + 1, np.int32)
            np.cumsum([len(x) for x in self.dvals], out=offs[1:])
            return {"offsets": offs, "chars": np.frombuffer(b"".join(self.dvals), np.uint8), "width": 0, "n_entries": self.n_dict}
        return {"values": np.ascontiguousarray(self.dvals, np.uint8).ravel(), "width": self.chunk.width, "n_entries": self.n_dict}

    def counts(self):
        """(blocks on the fast path, pages on the slow path) of this chunk when it is kept."""
        if not self.kept:
            return 0, 0
        return (sum(b for p, b in self.paths if p == "fast"), sum(b for p, b in self.paths if p == "slow"))


class Plain:
    """A chunk without a dictionary (BOOLEAN, DELTA): never eligible."""

    def __init__(self, chunk):
        self.chunk, self.kept, self.keep, self.eligible = chunk, False, True, False

    def counts(self):
        return 0, 0


class Case:
    def __init__(self, name, build, bad=False):
        self.name, self.build, self.bad = name, build, bad


def _noreps(ids, n_dict):
    """Break chance repeats, so that packed runs are cut only where a case puts an RLE run."""
    if n_dict < 4:
        return ids
    return (ids + np.arange(len(ids), dtype=np.uint64) % 2 * 3) % np.uint64(n_dict)


def _cases():
    out = []

    # ---- entry counts at thread-group and block edges, one page each, every type
    for tname in TYPES:
        def build(compress, tname=tname):
            rng = np.random.default_rng(len(tname))
            specs = []
            for n in COUNTS:
                s = Spec(f"{tname}_{n}", tname, make_dict(tname, 25, rng), compress=compress)
                s.page(rng.integers(0, 25, n), seed=n)
                specs.append(s)
            return specs
        out.append(Case(f"counts-{tname}", build))

    # ---- dictionary sizes: id width 0, the index width's thresholds, strings
    def dict_sizes(compress):
        rng = np.random.default_rng(21)
        specs = []
        for nd in (1, 2, 255, 256, 257, 65536, 65537):
            s = Spec(f"i32_{nd}", "int32", make_dict("int32", nd, rng), compress=compress)
            ids = rng.integers(0, nd, 4097)
            ids[0], ids[-1] = nd - 1, 0
            s.page(ids, seed=nd)
            specs.append(s)
        for nd, strings in ((1, "mixed"), (2, "mixed"), (257, "mixed"), (256, "short")):
            s = Spec(f"str_{nd}_{strings}", "binary", make_dict("binary", nd, rng, strings), compress=compress)
            ids = rng.integers(0, nd, 4097)
            ids[0], ids[-1] = nd - 1, 0
            s.page(ids, seed=nd)
            specs.append(s)
        return specs
    out.append(Case("dictionary-sizes", dict_sizes))

    def empty_dict(compress):
        specs = []
        for tname in ("int32", "binary", "flba5"):
            for lname in ("a", "e"):
                s = Spec(f"empty_{tname}_{lname}", tname, make_dict(tname, 0, np.random.default_rng(0)), optional=True,
                         layout=K.LAYOUTS[lname], compress=compress)
                s.page([], bw=0, present=np.zeros(5000, bool))
                specs.append(s)
        return specs
    out.append(Case("empty-dictionary-all-null", empty_dict))

    # ---- id widths the dictionary does not need
    for bw in (8, 13, 32):
        def build(compress, bw=bw):
            rng = np.random.default_rng(bw)
            specs = []
            for tname in ("int64", "binary"):
                for n in (17, 4097):
                    s = Spec(f"{tname}_w{bw}_{n}", tname, make_dict(tname, 7, rng), compress=compress)
                    s.page(rng.integers(0, 7, n), bw=bw, seed=n)
                    specs.append(s)
            return specs
        out.append(Case(f"id-width-{bw}", build))

    # ---- page layouts: v1 / v2, Snappy / uncompressed, BIT_PACKED levels, PLAIN_DICTIONARY pages
    for lname, lay in (("a", K.LAYOUTS["a"]), ("b", K.LAYOUTS["b"]), ("c", K.LAYOUTS["c"]), ("d", K.LAYOUTS["d"]), ("e", K.LAYOUTS["e"]),
                       ("v1s", V1S)):
        def build(compress, lay=lay):
            rng = np.random.default_rng(31)
            specs = []
            for tname in ("double", "binary"):
                for optional in (False, True):
                    s = Spec(f"{tname}_{int(optional)}", tname, make_dict(tname, 25, rng), optional=optional, layout=lay, compress=compress)
                    for n in (17, 4097):
                        present = rng.random(n) < 0.8 if optional else None
                        s.page(rng.integers(0, 25, int(present.sum()) if optional else n), present=present, seed=n)
                    specs.append(s)
            return specs
        out.append(Case(f"layout-{lname}", build))

    def plain_dictionary(compress):
        rng = np.random.default_rng(32)
        specs = []
        for tname in ("int32", "binary"):
            s = Spec(f"pd_{tname}", tname, make_dict(tname, 7, rng), compress=compress, dict_encoding=K.PLAIN_DICTIONARY)
            for n in (17, 4097):
                s.page(rng.integers(0, 7, n), encoding=K.PLAIN_DICTIONARY, seed=n)
            specs.append(s)
        return specs
    out.append(Case("plain-dictionary-pages", plain_dictionary))

    # ---- run shapes
    def styles(compress):
        rng = np.random.default_rng(41)
        specs = []
        for style, counts in (("mr", (17, 4097)), ("rle", (1, 17, 200)), ("mixed", (17, 300))):
            for tname in ("int64", "binary"):
                for optional in (False, True):
                    for n in counts:
                        s = Spec(f"{style}_{tname}_{int(optional)}_{n}", tname, make_dict(tname, 7, rng), optional=optional, compress=compress)
                        present = rng.random(n) < 0.8 if optional else None
                        ids = rng.integers(0, 7, int(present.sum()) if optional else n)
                        if style == "mr" and n > 100:
                            ids[40:90] = 3          # an RLE run between the packed groups
                        s.page(ids, style=style, present=present, seed=n)
                        specs.append(s)
        return specs
    out.append(Case("run-styles", styles))

    def rle_three_blocks(compress):
        rng = np.random.default_rng(42)
        specs = []
        for tname in ("int32", "binary"):
            n = 3 * FBLK + 100
            ids = rng.integers(0, 7, n).astype(np.uint64)
            ids[FBLK - 50:2 * FBLK + 50] = 5          # one RLE run over the end of block 0, block 1, the start of block 2
            s = Spec(f"rle3_{tname}", tname, make_dict(tname, 7, rng), compress=compress)
            s.page(ids)
            specs.append(s)
        return specs
    out.append(Case("rle-run-over-three-blocks", rle_three_blocks))

    def boundary_on_block(compress):
        rng = np.random.default_rng(43)
        specs = []
        for first_rle in (False, True):
            n = 2 * FBLK + 9
            ids = _noreps(rng.integers(0, 25, n).astype(np.uint64), 25)
            if first_rle:
                ids[:FBLK] = 11                    # an RLE run that ends exactly where block 1 starts
            else:
                ids[FBLK:FBLK + 64] = 11           # packed groups up to the block boundary, an RLE run from it
            s = Spec(f"edge_{int(first_rle)}", "int64", make_dict("int64", 25, rng), compress=compress)
            s.page(ids)
            specs.append(s)
        return specs
    out.append(Case("run-boundary-on-block-boundary", boundary_on_block))

    def too_many_runs(compress):
        rng = np.random.default_rng(44)
        specs = []
        for tname, optional in (("int32", False), ("binary", False), ("binary", True)):
            n = 4097
            present = rng.random(n) < 0.8 if optional else None
            s = Spec(f"many_{tname}_{int(optional)}", tname, make_dict(tname, 7, rng), optional=optional, compress=compress)
            s.page(rng.integers(0, 7, int(present.sum()) if optional else n), style="mixed", present=present)   # > 1000 runs
            assert s.paths[-1][0] == "slow"
            specs.append(s)
        return specs
    out.append(Case("more-runs-than-the-table", too_many_runs))

    # ---- nulls
    def nulls(compress):
        rng = np.random.default_rng(51)
        specs = []
        n = 5000
        shapes = {
            "all_present": np.ones(n, bool),
            "random80": rng.random(n) < 0.8,
            "first_null": np.arange(n) != 0,
            "last_null": np.arange(n) != n - 1,
            "alternating": np.arange(n) % 2 == 0,          # bit-packed levels
            "all_null": np.zeros(n, bool),
        }
        for tname in ("int32", "double", "flba5", "binary"):
            for lname in ("a", "c"):
                for sname, present in shapes.items():
                    s = Spec(f"{sname}_{tname}_{lname}", tname, make_dict(tname, 300 if tname == "int32" else 7, rng), optional=True,
                             layout=K.LAYOUTS[lname], compress=compress)
                    s.page(rng.integers(0, s.n_dict, int(present.sum())), present=present, seed=len(sname))
                    specs.append(s)
        return specs
    out.append(Case("nulls", nulls))

    def many_level_runs(compress):
        rng = np.random.default_rng(52)
        specs = []
        for tname in ("int64", "binary"):
            n = 5000
            present = rng.random(n) < 0.5
            s = Spec(f"lvlruns_{tname}", tname, make_dict(tname, 7, rng), optional=True, compress=compress)
            s.page(rng.integers(0, 7, int(present.sum())), present=present, level_style="mixed")   # ~ n / 3.5 level runs > n / 8 + 64
            assert s.paths[-1][0] == "slow"
            specs.append(s)
        return specs
    out.append(Case("more-level-runs-than-the-table", many_level_runs))

    def small_optional_v2(compress):
        """Fewer than 8 entries, every one present, in a v2 page: bit-packed levels and num_nulls = 0, so no level table."""
        rng = np.random.default_rng(53)
        s = Spec("small_v2", "int32", make_dict("int32", 7, rng), optional=True, layout=K.LAYOUTS["e"], compress=compress)
        s.page(rng.integers(0, 7, 5))
        assert s.paths[-1][0] == "slow"
        t = Spec("small_v1", "int32", make_dict("int32", 7, rng), optional=True, layout=K.LAYOUTS["a"], compress=compress)
        t.page(rng.integers(0, 7, 5))
        assert t.paths[-1][0] == "fast"
        return [s, t]
    out.append(Case("few-entries-bit-packed-levels", small_optional_v2))

    # ---- several pages per chunk: page starts that are no multiple of 4, 16 or 32
    def pages(compress):
        rng = np.random.default_rng(61)
        specs = []
        for nd in (25, 300):                      # index widths 1 and 2
            for tname in ("int64", "binary"):
                for optional in (False, True):
                    for lname in ("a", "c"):
                        s = Spec(f"pages_{nd}_{tname}_{int(optional)}_{lname}", tname, make_dict(tname, nd, rng, "short"), optional=optional,
                                 layout=K.LAYOUTS[lname], compress=compress)
                        for n in (33, 4095, 1, 17, 9003):
                            present = rng.random(n) < 0.8 if optional else None
                            if optional and n == 1:
                                present = np.zeros(1, bool)
                            s.page(rng.integers(0, nd, int(present.sum()) if optional else n), present=present, seed=n)
                        specs.append(s)
        return specs
    out.append(Case("several-pages", pages))

    def pages_width4(compress):
        rng = np.random.default_rng(62)
        s = Spec("pages_w4", "int32", make_dict("int32", 65537, rng), optional=True, compress=compress)
        for n in (33, 4095, 1, 17, 9003):
            present = rng.random(n) < 0.8
            ids = rng.integers(0, 65537, int(present.sum()))
            if len(ids):
                ids[-1] = 65536
            s.page(ids, present=present, seed=n)
        return [s]
    out.append(Case("several-pages-index-width-4", pages_width4))

    # ---- ineligible chunks: decoded as ever
    def ineligible(compress):
        rng = np.random.default_rng(71)
        specs = []
        for tname in ("int64", "binary"):
            s = Spec(f"fallback_{tname}", tname, make_dict(tname, 25, rng), compress=compress)
            s.page(rng.integers(0, 25, 4097))
            s.page(rng.integers(0, 25, 17), seed=1)
            s.plain_page(300, rng)
            specs.append(s)
        b = K.Chunk("flag", K.BOOLEAN, compress=compress)
        bv = rng.integers(0, 2, (1000, 1)).astype(np.uint8)
        b.add_page(K.PLAIN, K.plain(K.BOOLEAN, bv), vals=bv)
        specs.append(Plain(b))
        d = K.Chunk("delta", K.INT64, compress=compress)
        dv = np.cumsum(rng.integers(-50, 50, 1000)).astype(np.int64)
        d.add_page(K.DELTA_BINARY_PACKED, K.dbp(dv), vals=dv.view(np.uint8).reshape(-1, 8))
        specs.append(Plain(d))
        return specs
    out.append(Case("ineligible-chunks", ineligible))

    # ---- a batch mixing kept chunks, eligible chunks that are not asked for, and ineligible ones
    def mixed(compress):
        rng = np.random.default_rng(81)
        specs = []
        for k, (tname, optional, keep) in enumerate((("int64", True, True), ("binary", False, False), ("binary", True, True),
                                                     ("double", False, False), ("flba16", True, True))):
            s = Spec(f"mix_{k}", tname, make_dict(tname, 25, rng), optional=optional, layout=K.LAYOUTS["c" if k % 2 else "a"], compress=compress)
            for n in (4097, 33):
                present = rng.random(n) < 0.8 if optional else None
                s.page(rng.integers(0, 25, int(present.sum()) if optional else n), present=present, seed=n)
            s.keep = keep
            specs.append(s)
        f = Spec("mix_fallback", "binary", make_dict("binary", 25, rng), compress=compress)
        f.page(rng.integers(0, 25, 100))
        f.plain_page(50, rng)
        specs.append(f)
        return specs
    out.append(Case("mixed-batch", mixed))

    # ---- an id equal to n_entries: in a bit-packed run, and as the value of an RLE run
    for where, pos in (("first", 100), ("middle", FBLK + 2000), ("last", 2 * FBLK + 30)):
        for kind in ("packed", "rle"):
            def bad(compress, pos=pos, kind=kind):
                rng = np.random.default_rng(91)
                specs = []
                for tname, optional in (("binary", False), ("int64", False), ("int64", True)):
                    n = 2 * FBLK + 100
                    present = (np.arange(n) % 5 != 4) if optional else None
                    nv = int(present.sum()) if optional else n
                    ids = _noreps(rng.integers(0, 7, nv).astype(np.uint64), 7)
                    p = min(pos, nv - 30)
                    good_ids = ids.copy()
                    if kind == "rle":
                        ids[p:p + 24] = 7              # 24 repeats: an RLE run whatever the packed groups before it take
                        good_ids[p:p + 24] = 6
                    else:
                        ids[p] = 7
                        good_ids[p] = 6
                    for name, use in (("good", good_ids), ("bad", ids)):
                        s = Spec(f"{name}_{tname}_{int(optional)}", tname, make_dict(tname, 7, rng), optional=optional, compress=compress)
                        s.page(use, bw=3, present=present)
                        s.is_bad = name == "bad"
                        specs.append(s)
                return specs
            out.append(Case(f"bad-id-{kind}-{where}-block", bad, bad=True))
    return out


CASES = {c.name: c for c in _cases()}
