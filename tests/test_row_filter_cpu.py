"""Row filters on the host (no GPU): the planner and the comparisons of pf_decode_row_group_filter in a stand-alone
program under AddressSanitizer + UBSan (tests/native/pf_filter_check.cpp), pfloor.predicate's PLAIN-bytes conversion,
and the reference the GPU tests rely on (filter_cases.eval_predicates / take_rows) against pyarrow.compute."""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import filter_cases as FC
import window_cases as WC
from conftest import GOLDEN, ROOT

CSRC = os.path.join(ROOT, "parquet-floor_amd", "csrc")


def test_planner_and_comparisons_under_asan(tmp_path):
    exe = tmp_path / "pf_filter_check"
    cmd = ["g++", "-std=c++17", "-O0", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-static-libasan", "-static-libubsan", "-I", os.path.join(ROOT, "include"), "-I", CSRC,
           os.path.join(ROOT, "tests", "native", "pf_filter_check.cpp"), os.path.join(CSRC, "pf_plan.cpp"), "-o", str(exe)]
    subprocess.run(cmd, check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=97",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=98")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    words = r.stdout.split()
    assert words[-4] == "checks" and int(words[-3]) > 200 and words[-2:] == ["failures", "0"], r.stdout[-500:]


# ---- pfloor.predicate ------------------------------------------------------------------------------------------------

def test_plain_bytes_of_every_type():
    from pfloor import predicate as P
    assert P.plain_bytes(True, P.BOOLEAN) == b"\x01" and P.plain_bytes(False, P.BOOLEAN) == b"\x00" and P.plain_bytes(1, P.BOOLEAN) == b"\x01"
    assert P.plain_bytes(-2, P.INT32) == b"\xfe\xff\xff\xff" and P.plain_bytes(2**31 - 1, P.INT32) == b"\xff\xff\xff\x7f"
    assert P.plain_bytes(-2**31, P.INT32) == b"\x00\x00\x00\x80"
    assert P.plain_bytes(-2**63, P.INT64) == b"\x00" * 7 + b"\x80" and P.plain_bytes(2**63 - 1, P.INT64) == b"\xff" * 7 + b"\x7f"
    assert P.plain_bytes(258, P.INT64) == b"\x02\x01" + b"\x00" * 6
    assert P.plain_bytes(1.5, P.FLOAT) == struct.pack("<f", 1.5) and P.plain_bytes(-0.0, P.DOUBLE) == struct.pack("<d", -0.0)
    assert P.plain_bytes(3, P.DOUBLE) == struct.pack("<d", 3.0)
    assert P.plain_bytes(float("inf"), P.FLOAT) == struct.pack("<f", math.inf)
    assert struct.unpack("<d", P.plain_bytes(float("nan"), P.DOUBLE))[0] != struct.unpack("<d", P.plain_bytes(float("nan"), P.DOUBLE))[0]
    assert P.plain_bytes("né", P.BYTE_ARRAY) == "né".encode() and P.plain_bytes(b"a\x00\xff", P.BYTE_ARRAY) == b"a\x00\xff"
    assert P.plain_bytes(bytearray(b""), P.BYTE_ARRAY) == b""
    for value, ptype in ((2**31, P.INT32), (-2**31 - 1, P.INT32), (2**63, P.INT64), (-2**63 - 1, P.INT64), (1.5, P.INT32), ("1", P.INT64),
                         (True, P.INT32), (2, P.BOOLEAN), ("x", P.BOOLEAN), (b"1", P.DOUBLE), (True, P.FLOAT), (1e39, P.FLOAT),
                         (5, P.BYTE_ARRAY), (None, P.BYTE_ARRAY), (1, P.INT96), (b"12345", P.FIXED_LEN_BYTE_ARRAY)):
        with pytest.raises(ValueError):
            P.plain_bytes(value, ptype)


def test_predicates_bind_to_chunks():
    from pfloor import predicate as P
    from pfloor.decoder import ParquetFile
    with ParquetFile(WC.fixture_path("rw_none")) as f:   # key INT64, s optional string, l list<int32>
        cols = f.columns
        assert [P.resolve(cols, c) for c in (0, "key", "s", 1, "l")] == [0, 0, 1, 1, 2]
        for bad in ("nope", 3, -1):
            with pytest.raises(ValueError):
                P.resolve(cols, bad)
        preds = [P.Range("key", 5, None), P.Eq("s", "w1"), P.IsNull(1), P.NotNull("key"), P.Range(0)]
        got = P.bind(preds, cols, {0: 1, 1: 0})
        assert got == [(1, 0, (5).to_bytes(8, "little"), None), (0, 0, b"w1", b"w1"), (0, 1, None, None), (1, 2, None, None),
                       (1, 0, None, None)]
        with pytest.raises(ValueError):
            P.bind([P.Eq("key", 2**63)], cols, {0: 0})
        with pytest.raises(ValueError):
            P.Eq("key", None)
        assert "Eq('s', 'w1')" in repr(preds[1]) and "IsNull(1)" in repr(preds[2])


# ---- the reference against pyarrow.compute ----------------------------------------------------------------------------

def _arrow_columns(t, names):
    out = []
    for name in names:
        col = t.column(name)
        v = col.to_pylist()
        import pyarrow as pa
        ty = col.type
        if pa.types.is_string(ty) or pa.types.is_binary(ty) or pa.types.is_large_string(ty):
            out.append((WC.canonical_strings(v, True), FC.BYTE_ARRAY))
        elif pa.types.is_int64(ty):
            out.append((WC.canonical_fixed(v, np.int64, True), FC.INT64))
        elif pa.types.is_int32(ty):
            out.append((WC.canonical_fixed(v, np.int32, True), FC.INT32))
        elif pa.types.is_float64(ty):
            out.append((WC.canonical_fixed(v, np.float64, True), FC.DOUBLE))
        else:
            raise AssertionError(ty)
    return out


def _check_against_arrow(t, names, preds, arrow_mask):
    pc = pytest.importorskip("pyarrow.compute")
    cols = _arrow_columns(t, names)
    mask = FC.eval_predicates(cols, preds)
    want = np.array(pc.fill_null(arrow_mask, False).to_pylist(), bool)
    assert np.array_equal(mask, want), (preds, np.flatnonzero(mask != want)[:8])
    part = _arrow_columns(t.filter(pc.fill_null(arrow_mask, False)), names)
    idx = np.flatnonzero(mask)
    for c, ((whole, _t), (exp, _t2)) in enumerate(zip(cols, part)):
        WC.assert_window_equal(FC.take_rows(whole, idx), exp, f"{preds} col {names[c]}")
    return int(mask.sum())


@pytest.mark.parametrize("name", WC.FIXTURES)
def test_reference_agrees_with_pyarrow_on_the_window_fixtures(name):
    pq = pytest.importorskip("pyarrow.parquet")
    pc = pytest.importorskip("pyarrow.compute")
    t = pq.read_table(WC.fixture_path(name), columns=["key", "s"])
    key, s = t.column("key"), pc.cast(t.column("s"), "binary")
    keys = key.to_pylist()
    k_lo, k_hi = sorted(keys)[len(keys) // 4], sorted(keys)[len(keys) // 2]
    some = next(x for x in t.column("s").to_pylist() if x)
    seen = set()
    for preds, m in (
            ([(0, FC.RANGE, k_lo, None)], pc.greater_equal(key, k_lo)),
            ([(0, FC.RANGE, k_lo, k_hi)], pc.and_(pc.greater_equal(key, k_lo), pc.less_equal(key, k_hi))),
            ([(0, FC.RANGE, keys[7], keys[7])], pc.equal(key, keys[7])),
            ([(0, FC.RANGE, None, min(keys) - 1)], pc.less_equal(key, min(keys) - 1)),
            ([(1, FC.IS_NULL, None, None)], pc.is_null(s)),
            ([(1, FC.NOT_NULL, None, None), (0, FC.RANGE, None, k_hi)], pc.and_(pc.is_valid(s), pc.less_equal(key, k_hi))),
            ([(1, FC.RANGE, some.encode(), some.encode())], pc.equal(s, some.encode())),
            ([(1, FC.RANGE, some.encode()[:1], None)], pc.greater_equal(s, some.encode()[:1])),
            ([(1, FC.RANGE, None, None)], pc.is_valid(s)),
            ([(0, FC.RANGE, None, None)], pc.is_valid(key))):
        seen.add(_check_against_arrow(t, ["key", "s"], preds, m))
    assert 0 in seen and t.num_rows in seen and len(seen) > 5


def test_reference_agrees_with_pyarrow_on_lineitem():
    pq = pytest.importorskip("pyarrow.parquet")
    pc = pytest.importorskip("pyarrow.compute")
    import pyarrow as pa
    t = pq.read_table(os.path.join(GOLDEN, "c2_lineitem.parquet"))
    names = [f.name for f in t.schema if pa.types.is_int64(f.type) or pa.types.is_int32(f.type) or pa.types.is_float64(f.type) or
             pa.types.is_string(f.type)]
    ints = [n for n in names if pa.types.is_integer(t.schema.field(n).type)]
    dbls = [n for n in names if pa.types.is_float64(t.schema.field(n).type)]
    strs = [n for n in names if pa.types.is_string(t.schema.field(n).type)]
    assert ints and dbls and strs
    i, d, s = names.index(ints[0]), names.index(dbls[0]), names.index(strs[0])
    iv, dv = sorted(t.column(ints[0]).to_pylist()), sorted(t.column(dbls[0]).to_pylist())
    sv = sorted(t.column(strs[0]).to_pylist())
    ilo, dlo, dhi, smid = iv[len(iv) // 2], dv[len(dv) // 4], dv[3 * len(dv) // 4], sv[len(sv) // 2].encode()
    sb = pc.cast(t.column(strs[0]), "binary")
    n1 = _check_against_arrow(t, names, [(i, FC.RANGE, ilo, None), (d, FC.RANGE, dlo, dhi)],
                              pc.and_(pc.greater_equal(t.column(ints[0]), ilo),
                                      pc.and_(pc.greater_equal(t.column(dbls[0]), dlo), pc.less_equal(t.column(dbls[0]), dhi))))
    n2 = _check_against_arrow(t, names, [(s, FC.RANGE, None, smid), (i, FC.NOT_NULL, None, None)],
                              pc.and_(pc.less_equal(sb, smid), pc.is_valid(t.column(ints[0]))))
    assert 0 < n1 < t.num_rows and 0 < n2 <= t.num_rows


# ---- pruning by the page index ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", WC.FIXTURES + ("rw_keys",))
def test_prune_row_group_against_the_page_index(name):
    """The hull of the pages whose [min, max] meets the bounds, recomputed here from page_index()."""
    from pfloor import predicate as P
    from pfloor.decoder import ParquetFile
    with ParquetFile(WC.fixture_path(name)) as f:
        n = f.row_group_rows(0)
        px = f.page_index(0, 0)
        first = [r for _o, _s, r in px["offset_index"]]
        pages = WC.page_rows(first, n)
        ci = px["column_index"]
        mins = [int.from_bytes(b, "little", signed=True) for b in ci["min_values"]]
        maxs = [int.from_bytes(b, "little", signed=True) for b in ci["max_values"]]
        assert f.columns[0].physical_type == 2 and not any(ci["null_pages"])

        def hull(lo, hi, a=0, b=n):
            keep = [p for p in range(len(pages)) if (lo is None or maxs[p] >= lo) and (hi is None or mins[p] <= hi)]
            if not keep:
                return None
            a, b = max(a, pages[keep[0]][0]), min(b, pages[keep[-1]][1])
            return (a, b) if a < b else None
        probes = [(mins[2], mins[2]), (maxs[1], mins[3]), (None, mins[0] - 1), (maxs[-1] + 1, None), (None, None), (mins[1] + 1, mins[1] + 1),
                  (min(mins), max(maxs)), (maxs[4], None), (None, mins[2])]
        for lo, hi in probes:
            pred = P.Eq(0, lo) if lo is not None and lo == hi else P.Range(0, lo, hi)
            assert f.prune_row_group(0, [pred]) == hull(lo, hi), (name, lo, hi)
            assert f.prune_row_group(0, [pred], 130, 1000) == hull(lo, hi, 130, 1000), (name, lo, hi)
            assert f.prune_row_group(0, [pred, P.NotNull(0), P.IsNull(1)]) == hull(lo, hi)
        # a conjunction intersects the hulls; predicates the index cannot use leave the range whole
        both = [P.Range(0, mins[1], None), P.Range(0, None, maxs[3])]
        h1, h2 = hull(mins[1], None), hull(None, maxs[3])
        a, b = max(h1[0], h2[0]), min(h1[1], h2[1])
        assert f.prune_row_group(0, both) == ((a, b) if a < b else None)
        assert f.prune_row_group(0, [P.IsNull(1), P.NotNull(0)]) == (0, n) and f.prune_row_group(0, []) == (0, n)
        assert f.prune_row_group(0, [P.IsNull(1)], 5, 9) == (5, 9)
        assert f.bloom_probe(0, 0, b"\x00" * 8) is None   # pyarrow wrote no Bloom filter


def test_new_structs_match_the_header(tmp_path):
    """pf_predicate and pf_selection_info: the ctypes mirrors against sizeof / offsetof from include/pfloor.h."""
    import ctypes as C
    from pfloor import _native
    structs = {"pf_predicate": _native.Predicate, "pf_selection_info": _native.SelectionInfo}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pfloor.h"', "int main(void){"]
    for cname, py in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for f, _ in py._fields_:
            lines.append(f'printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));')
    lines.append('printf("max %d 0\\n", PF_MAX_PREDICATES * 100 + PF_PRED_RANGE * 10 + PF_PRED_IS_NULL + PF_PRED_NOT_NULL * 10);')
    lines.append("return 0;}")
    src = tmp_path / "probe.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = {}
    for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines():
        s, f, v = ln.split()
        got[(s, f)] = int(v)
    for cname, py in structs.items():
        assert got[(cname, "size")] == C.sizeof(py), cname
        for f, _ in py._fields_:
            assert got[(cname, f)] == getattr(py, f).offset, (cname, f)
    assert ("max", "821") in got and (_native.PF_MAX_PREDICATES, _native.PRED_RANGE, _native.PRED_IS_NULL, _native.PRED_NOT_NULL) == (8, 0, 1, 2)
