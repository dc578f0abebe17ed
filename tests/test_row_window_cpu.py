"""Row ranges on the host (no GPU): pf_file_chunk_desc_rows selects pages through the OffsetIndex and reads nothing
else of the chunk; ParquetFile.candidate_rows turns a ColumnIndex into row ranges; the reference slicer the GPU tests
rely on (window_cases.slice_chunk) agrees with pyarrow's Table.slice."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import window_cases as WC
from conftest import GOLDEN, ROOT
from pfloor._native import ChunkDesc, ChunkRows, PageDesc, lib
from pfloor.decoder import ParquetFile

CSRC = os.path.join(ROOT, "parquet-floor_amd", "csrc")
PAGE_FIELDS = [f for f, _ in PageDesc._fields_]


def pages_of(d):
    return [{f: getattr(d.pages[i], f) for f in PAGE_FIELDS} for i in range(d.n_pages)]


def desc_tuple(d):
    return ([getattr(d, f) for f in ("physical_type", "type_length", "max_def", "max_rep", "repeated_def", "list_null_def",
                                     "codec", "n_pages", "chunk_offset", "chunk_size", "num_rows")], pages_of(d))


def rows_tuple(r):
    return [getattr(r, f) for f, _ in ChunkRows._fields_]


def ranges_for(first, n):
    """The issue's ranges, from the chunk's own page edges (first: first row of every data page)."""
    e = first[1:]   # inner page edges
    assert len(e) >= 4
    return {"empty at 0": (0, 0), "first row": (0, 1), "whole": (0, n), "last row": (n - 1, n), "empty at n": (n, n),
            "inside one page": (e[0] + 3, e[1] - 3), "ends on an edge": (e[0] + 5, e[1]), "starts on an edge": (e[1], e[1] + 7),
            "crosses one edge": (e[1] - 2, e[1] + 2), "crosses three edges": (e[0] - 1, e[2] + 1),
            "empty inside a page": (e[0] + 3, e[0] + 3)}


@pytest.mark.parametrize("name", WC.FIXTURES)
def test_pages_selected_by_the_offset_index(name):
    with ParquetFile(WC.fixture_path(name)) as f:
        n = f.row_group_rows(0)
        for col in range(f.num_columns):
            start, size = f.chunk_range(0, col)
            oi = f.page_index(0, col)["offset_index"]
            first = [r for _o, _s, r in oi]
            full = f.chunk_desc(0, col, 0)
            full_pages = pages_of(full)
            has_dict = full_pages[0]["page_type"] == 2
            assert len(full_pages) == len(oi) + has_dict
            for label, (lo, hi) in ranges_for(first, n).items():
                d, r = f.chunk_desc_rows(0, col, lo, hi, 512)
                sel = WC.select_pages(first, n, lo, hi)
                what = f"{name} c{col} {label} [{lo}, {hi})"
                assert r.indexed == 1 and r.n_data_pages == len(sel), what
                assert r.take_rows == hi - lo and r.first_row + r.skip_rows == lo, what
                if not sel:
                    assert (d.n_pages, d.chunk_size, d.num_rows, r.dict_size, r.data_size, r.skip_rows) == (0, 0, 0, 0, 0, 0), what
                    continue
                p0, p1 = sel[0], sel[-1]
                assert sel == list(range(p0, p1 + 1)) and r.first_page == p0, what
                assert r.first_row == first[p0] and r.skip_rows == lo - first[p0], what
                assert (r.dict_start, r.dict_size) == ((start, oi[0][0] - start) if has_dict else (start, 0)), what
                assert (r.data_start, r.data_size) == (oi[p0][0], oi[p1][0] + oi[p1][1] - oi[p0][0]), what
                assert start <= r.data_start and r.data_start + r.data_size <= start + size, what
                last_row = first[p1 + 1] if p1 + 1 < len(first) else n
                assert (d.chunk_offset, d.chunk_size, d.num_rows) == (512, r.dict_size + r.data_size, last_row - first[p0]), what
                # the descriptor's pages are pf_file_chunk_desc's, offsets rebased into the two-range buffer
                want = []
                if has_dict:
                    want.append(dict(full_pages[0]))
                for p in sel:
                    e = dict(full_pages[p + has_dict])
                    e["offset"] = e["offset"] - (oi[p0][0] - start) + r.dict_size
                    want.append(e)
                assert pages_of(d) == want, what
            # a call does not disturb the descriptor pf_file_chunk_desc returned
            assert pages_of(full) == full_pages


@pytest.mark.parametrize("name", WC.FIXTURES)
def test_no_byte_outside_the_two_ranges_is_read(name, tmp_path):
    src = WC.fixture_path(name)
    with ParquetFile(src) as f:
        n = f.row_group_rows(0)
        cases = []
        for col in range(f.num_columns):
            start, size = f.chunk_range(0, col)
            first = [r for _o, _s, r in f.page_index(0, col)["offset_index"]]
            for label in ("inside one page", "crosses three edges", "last row"):
                lo, hi = ranges_for(first, n)[label]
                d, r = f.chunk_desc_rows(0, col, lo, hi, 0)
                cases.append((col, lo, hi, start, size, desc_tuple(d), rows_tuple(r), desc_tuple(f.chunk_desc(0, col, 0))))
    raw = np.fromfile(src, np.uint8)
    for k, (col, lo, hi, start, size, want_d, want_r, whole) in enumerate(cases):
        poisoned = raw.copy()
        keep = np.zeros(len(raw), bool)
        keep[want_r[6]:want_r[6] + want_r[7]] = True     # dict_start, dict_size
        keep[want_r[8]:want_r[8] + want_r[9]] = True     # data_start, data_size
        chunk = np.zeros(len(raw), bool)
        chunk[start:start + size] = True
        assert (chunk & ~keep).any()
        poisoned[chunk & ~keep] = 0xFF
        path = str(tmp_path / f"poison{k}.parquet")
        poisoned.tofile(path)
        with ParquetFile(path) as g:
            d, r = g.chunk_desc_rows(0, col, lo, hi, 0)
            assert desc_tuple(d) == want_d and rows_tuple(r) == want_r
            try:
                differs = desc_tuple(g.chunk_desc(0, col, 0)) != whole
            except Exception:
                differs = True
            assert differs, "the whole-chunk walk did not notice the poison: the test proves nothing"


def test_chunk_without_offset_index_lists_every_page():
    with ParquetFile(os.path.join(GOLDEN, "c5_nested.parquet")) as f:
        for col in range(f.num_columns):
            n = f.row_group_rows(0)
            assert f.index_ranges(0, col)[1] is None
            start, size = f.chunk_range(0, col)
            whole = desc_tuple(f.chunk_desc(0, col, 64))
            lo, hi = n // 3, n // 3 + 5
            d, r = f.chunk_desc_rows(0, col, lo, hi, 64)
            assert desc_tuple(d) == whole
            n_data = sum(p["page_type"] != 2 for p in whole[1])
            assert rows_tuple(r) == [0, 0, n_data, 0, lo, hi - lo, 0, 0, start, size]


def test_argument_errors():
    L = lib()
    with ParquetFile(WC.fixture_path("rw_snappy")) as f:
        n = f.row_group_rows(0)
        d, r = ChunkDesc(), ChunkRows()
        for lo, hi in ((-1, 5), (5, 4), (0, n + 1), (n + 1, n + 1)):
            assert L.pf_file_chunk_desc_rows(f.h, 0, 0, lo, hi, 0, C.byref(d), C.byref(r)) == -1, (lo, hi)
        assert L.pf_file_chunk_desc_rows(f.h, 0, 0, 0, 1, 0, None, C.byref(r)) == -1
        assert L.pf_file_chunk_desc_rows(f.h, 0, 0, 0, 1, 0, C.byref(d), None) == -1
        assert L.pf_file_chunk_desc_rows(f.h, 1, 0, 0, 1, 0, C.byref(d), C.byref(r)) == -1
        assert L.pf_file_chunk_desc_rows(f.h, 0, f.num_columns, 0, 1, 0, C.byref(d), C.byref(r)) == -1
        assert L.pf_file_chunk_desc_rows(None, 0, 0, 0, 1, 0, C.byref(d), C.byref(r)) == -1


def test_damaged_index_is_corrupt_page(tmp_path):
    """A location moved outside the chunk, and a compressed_page_size cut below the page."""
    src = WC.fixture_path("rw_none")
    raw = np.fromfile(src, np.uint8)
    with ParquetFile(src) as f:
        (oi_off, oi_len) = f.index_ranges(0, 0)[1]
        oi = f.page_index(0, 0)["offset_index"]
    index = bytes(raw[oi_off:oi_off + oi_len])

    def zz(v):
        v = (v << 1) ^ (v >> 63)
        out = bytearray()
        while v >= 0x80:
            out.append((v & 0x7f) | 0x80)
            v >>= 7
        out.append(v)
        return bytes(out)
    off1, size1 = oi[1][0], oi[1][1]
    for label, old, new in (("offset past the chunk", zz(off1), zz(off1 + (1 << 20))[:len(zz(off1))]),
                            ("size below the page", zz(size1), zz(size1 - 40)[:len(zz(size1))])):
        assert len(old) == len(new) and index.count(old) >= 1
        at = index.index(old)
        bad = raw.copy()
        bad[oi_off + at:oi_off + at + len(new)] = np.frombuffer(new, np.uint8)
        path = str(tmp_path / "bad.parquet")
        bad.tofile(path)
        with ParquetFile(path) as g:
            d, r = ChunkDesc(), ChunkRows()
            rc = lib().pf_file_chunk_desc_rows(g.h, 0, 0, 0, g.row_group_rows(0), 0, C.byref(d), C.byref(r))
            assert rc == -2, (label, rc)


def test_sanitizer_run_over_index_and_header_mutations(tmp_path):
    exe = tmp_path / "pf_rows_fuzz"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           os.path.join(ROOT, "tests", "native", "pf_rows_fuzz.cpp"), os.path.join(CSRC, "pf_meta.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    work = tmp_path / "work"
    work.mkdir()
    r = subprocess.run([str(exe), WC.fixture_path("rw_snappy"), str(work)], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "calls" and words[4] == "direct" and int(words[5]) > 0   # (the header prefixes ran too)
    shutil.rmtree(work)


# ---- candidate_rows ------------------------------------------------------------------------------------------------

def _brute(values, present, lo, hi):
    return [i for i, (v, ok) in enumerate(zip(values, present)) if ok and (lo is None or v >= lo) and (hi is None or v <= hi)]


def _check_candidates(f, col, values, present, probes):
    n = f.row_group_rows(0)
    px = f.page_index(0, col)
    first = [r for _o, _s, r in px["offset_index"]]
    pages = WC.page_rows(first, n)
    for lo, hi in probes:
        got = f.candidate_rows(0, col, lo, hi)
        assert all(a < b for a, b in got) and all(x[1] < y[0] for x, y in zip(got, got[1:])), (lo, hi, got)   # merged, ascending
        for a, b in got:   # made of whole pages
            assert a in first and (b == n or b in first)
        inside = np.zeros(n, bool)
        for a, b in got:
            inside[a:b] = True
        hits = _brute(values, present, lo, hi)
        assert inside[hits].all(), f"col {col} [{lo}, {hi}]: matching rows {[h for h in hits if not inside[h]][:5]} not covered"
        # and no page is kept that the bounds exclude: a kept page's [min, max] meets [lo, hi]
        for (a, b) in pages:
            vals = [v for v, ok in zip(values[a:b], present[a:b]) if ok]
            if inside[a] and vals:
                assert (lo is None or max(vals) >= lo) and (hi is None or min(vals) <= hi), (col, lo, hi, a, b)
            if not vals:
                assert not inside[a], "a null page was kept"
    return pages


def _int_probes(values, pages):
    vs = sorted(values)
    edge = values[pages[2][0]]
    return [(None, None), (vs[0], vs[0]), (vs[-1], vs[-1]), (vs[0] - 10, vs[0] - 1), (vs[-1] + 1, vs[-1] + 9), (edge, edge),
            (edge - 1, edge + 1), (vs[len(vs) // 3], vs[len(vs) // 2]), (None, vs[5]), (vs[-5], None), (vs[7] + 0, vs[7] + 0),
            (vs[0] - 5, vs[-1] + 5)]


def test_candidate_rows_against_brute_force(oracle):
    path = WC.fixture_path("rw_keys")
    with oracle.open(path) as of, ParquetFile(path) as f:
        n = f.row_group_rows(0)
        for col, dt in ((0, np.int64), (1, np.int32), (3, np.int32)):
            a = of.decode(0, col)
            values = [int(v) for v in np.frombuffer(a["values"].tobytes(), dt)]
            present = list(WC._bits(a["validity"], n).astype(bool)) if "validity" in a else [True] * n
            first = [r for _o, _s, r in f.page_index(0, col)["offset_index"]]
            _check_candidates(f, col, values, present, _int_probes(values, WC.page_rows(first, n)))
        a = of.decode(0, 2)
        off, chars = a["offsets"], a["chars"].tobytes()
        names = [chars[off[i]:off[i + 1]] for i in range(n)]
        probes = [(None, None), (names[0], names[0]), (names[-1], names[-1]), (b"", b"m"), (b"n2", b"n21"), (b"zz", None),
                  (None, b"a"), (names[700], names[700]), (names[700][:4], names[700] + b"\x00"), (b"n1", b"n1")]
        _check_candidates(f, 2, names, [True] * n, probes)
    # the sorted key of the window fixtures: a one-value probe is exactly one page
    path = WC.fixture_path("rw_snappy")
    with oracle.open(path) as of, ParquetFile(path) as f:
        n = f.row_group_rows(0)
        keys = [int(v) for v in np.frombuffer(of.decode(0, 0)["values"].tobytes(), np.int64)]
        first = [r for _o, _s, r in f.page_index(0, 0)["offset_index"]]
        pages = WC.page_rows(first, n)
        for row in (0, 1, 200, 1500, n - 1):
            in_pages = [p for p in pages if keys[row] in keys[p[0]:p[1]]]
            if len(in_pages) == 1:
                assert f.candidate_rows(0, 0, keys[row], keys[row]) == in_pages
        assert f.candidate_rows(0, 0, keys[200], keys[200]) == [p for p in pages if p[0] <= 200 < p[1]]
        _check_candidates(f, 0, keys, [True] * n, _int_probes(keys, pages))


def test_candidate_rows_null_pages_truncated_bounds_and_types():
    class Stub(ParquetFile):
        def __init__(self, ptype, rows, oi, ci):
            self.columns = [type("Col", (), {"physical_type": ptype})()]
            self._rows, self._px = rows, {"offset_index": oi, "column_index": ci}

        def row_group_rows(self, rg):
            return self._rows

        def page_index(self, rg, col):
            return self._px

        def close(self):
            pass
    oi = [(4, 10, 0), (14, 10, 10), (24, 10, 25), (34, 10, 31)]
    ci = {"null_pages": [False, True, False, False], "min_values": [b"ab", b"", b"ab\xff", b"b"],
          "max_values": [b"ab", b"", b"ac", b"b\x80"], "boundary_order": 1, "null_counts": None}
    f = Stub(6, 40, oi, ci)
    assert f.candidate_rows(0, 0) == [(0, 10), (25, 40)]                       # the null page never
    assert f.candidate_rows(0, 0, b"ab", b"ab") == [(0, 10)]
    assert f.candidate_rows(0, 0, b"aba", b"aba") == []                       # "ab" < "aba" < "ab\xff": a prefix sorts first
    assert f.candidate_rows(0, 0, b"ab\xff\x00", b"ab\xff\x01") == [(25, 31)]
    assert f.candidate_rows(0, 0, b"abb", b"abz") == []                        # unsigned bytes: min "ab\xff" > "abz"
    assert f.candidate_rows(0, 0, b"b\x7f", None) == [(31, 40)]                 # a truncated max "b\x80" still bounds
    ints = {"null_pages": [False, False], "min_values": [(-5).to_bytes(8, "little", signed=True), (3).to_bytes(8, "little")],
            "max_values": [(2).to_bytes(8, "little"), (9).to_bytes(8, "little")], "boundary_order": 1, "null_counts": None}
    g = Stub(2, 20, [(4, 9, 0), (13, 9, 10)], ints)
    assert g.candidate_rows(0, 0, -3, -3) == [(0, 10)]                         # signed: -5 <= -3 <= 2
    assert g.candidate_rows(0, 0, 2, 3) == [(0, 20)]                           # adjacent pages merge
    assert g.candidate_rows(0, 0, 10, None) == []
    assert Stub(2, 20, None, ints).candidate_rows(0, 0, 1, 2) == [(0, 20)]
    assert Stub(2, 20, [(4, 9, 0), (13, 9, 10)], None).candidate_rows(0, 0, 1, 2) == [(0, 20)]
    for ptype in (0, 3, 4, 5, 7):
        with pytest.raises(ValueError):
            Stub(ptype, 20, [(4, 9, 0)], ints).candidate_rows(0, 0, 1, 2)


# ---- the reference slicer against pyarrow ---------------------------------------------------------------------------

def test_slicer_agrees_with_pyarrow_slice():
    pq = pytest.importorskip("pyarrow.parquet")
    t = pq.read_table(WC.fixture_path("rw_none"))
    n = t.num_rows

    def canon(tab):
        return (WC.canonical_fixed(tab.column("key").to_pylist(), np.int64, False),
                WC.canonical_strings(tab.column("s").to_pylist(), True),
                WC.canonical_list_int32(tab.column("l").to_pylist()))
    whole = canon(t)
    for skip, take in ((0, 0), (0, 1), (0, n), (n - 1, 1), (n, 0), (3, 61), (145, 149), (144, 2), (1001, 777), (5, -1)):
        part = canon(t.slice(skip, n - skip if take < 0 else take))
        for c in range(3):
            WC.assert_window_equal(WC.slice_chunk(whole[c], skip, take), part[c], f"col {c} window ({skip}, {take})")


def test_canonical_arrays_agree_with_the_oracle(oracle):
    """The fixtures' expected arrays: the oracle's whole-chunk decode equals the arrays the file was written from."""
    pq = pytest.importorskip("pyarrow.parquet")
    for name in WC.FIXTURES:
        t = pq.read_table(WC.fixture_path(name))
        want = (WC.canonical_fixed(t.column("key").to_pylist(), np.int64, False),
                WC.canonical_strings(t.column("s").to_pylist(), True), WC.canonical_list_int32(t.column("l").to_pylist()))
        with oracle.open(WC.fixture_path(name)) as of:
            for c in range(3):
                got = of.decode(0, c)
                assert got["status"] == 0, got["error"]
                WC.assert_window_equal(got, want[c], f"{name} col {c}")
