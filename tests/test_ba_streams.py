"""The PLAIN BYTE_ARRAY stream corpus (tests/ba_streams.py) on the CPU: the oracle and pyarrow read
every undamaged stream as the constructed values; the oracle's verdict on the damaged ones is what
test_gpu_ba_streams.py expects of the GPU; and the corpus is what it claims to be: the binary
families are full of positions that pass the value walk's candidate test away from any true prefix
(the text control is not), and the geometry cases land on the bytes they aim at."""
import importlib.util
import io
import os

import numpy as np
import pytest

import ba_streams as B
import pagekit as K
from conftest import GOLDEN
from golden_util import assert_chunk_equal

FILE_IDS = list(B.corpus())
_FILES = {}


@pytest.fixture(scope="session")
def ba_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("ba_streams"))


@pytest.fixture
def ba_file(oracle, ba_dir):
    """get(fid) -> {path, cases, info, chunks, expected, verdict}: the file of one corpus id, built once
    per session; verdict[c] is the oracle's status for chunk c."""
    def get(fid):
        if fid not in _FILES:
            cases = B.corpus()[fid]
            data, info, chunks, expected = B.build(cases, oracle.snappy_compress)
            path = os.path.join(ba_dir, fid + ".parquet")
            with open(path, "wb") as f:
                f.write(data)
            with oracle.open(path) as of:
                verdict = [of.decode(0, c)["status"] for c in range(len(cases))]
            _FILES[fid] = {"path": path, "cases": cases, "info": info, "chunks": chunks, "expected": expected,
                           "verdict": verdict}
        return _FILES[fid]
    return get


def _make_golden():
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(GOLDEN, "make_golden.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


# what the issue's CPU runs found, and the format: bytes after the last value are not read; a length that
# overruns the page, and a page that ends before its values do, are corrupt (PF_ERR_CORRUPT_PAGE = -2)
STATED_VERDICTS = {"trail_junk3": 0, "extra_record": 0, "last_overrun": -2}


@pytest.mark.parametrize("fid", FILE_IDS)
def test_oracle_and_pyarrow(oracle, ba_file, fid):
    import pyarrow.parquet as pq
    f = ba_file(fid)
    mg = _make_golden()
    n_ok = 0
    with oracle.open(f["path"]) as of:
        assert of.num_columns == len(f["cases"])
        for c, (case, exp) in enumerate(zip(f["cases"], f["expected"])):
            o = of.decode(0, c)
            assert o["status"] == f["verdict"][c]
            if case.damage:
                print(f"{fid} {case.describe()}: oracle status {o['status']} {o['error'] if o['status'] else ''}")
                if case.damage in STATED_VERDICTS:
                    assert o["status"] == STATED_VERDICTS[case.damage], case.describe()
                else:
                    assert o["status"] != 0, case.describe()
                if o["status"] != 0:
                    continue
            assert o["status"] == 0, (case.describe(), o["error"])
            assert_chunk_equal(o, exp, f"{fid} {case.name} [oracle vs construction]")
            n_ok += 1
            if case.damage:   # (pyarrow's verdict on bytes after the last value is its own)
                continue
            # pyarrow reads the chunk alone in a file of its own (a file's chunks here differ in row count)
            data, _info, _chunks, (exp1,) = B.build([case], oracle.snappy_compress)
            pf = pq.ParquetFile(io.BytesIO(data))
            pa_exp = mg.expected_for_column(pf.read_row_group(0), pf.metadata, 0)
            assert_chunk_equal(pa_exp, exp1, f"{fid} {case.name} [pyarrow vs construction]")
    print(f"{fid}: {n_ok} of {len(f['cases'])} chunks read, bit-exact with the construction")


def test_corpus_is_not_vacuous():
    """A stream stresses the walk only if positions other than the true prefixes pass its candidate
    test (the length fits, and so does the length after the value), and challenges link level 2 only if
    such positions chain three deep. Counted here from the format alone, before any GPU is involved."""
    for kind in B.FAMILIES + B.EXTRA:
        vals = B.family(kind)
        stream = K.plain(K.BYTE_ARRAY, vals)
        fit, _ = B.fitting(stream)
        false, chained = B.false_positions(stream, vals)
        per = false / len(vals)
        print(f"{kind}: {len(stream)} stream bytes, {len(vals)} values, {int(fit.sum())} positions that fit, "
              f"{false} false positions ({per:.2f} per value), {chained} at the end of a three-link false chain")
        assert len(stream) <= B.MAX_STREAM and len(stream) <= B.BA_SHORT * len(vals)
        if kind == "text":
            assert per < 1, (kind, per)
        elif kind in B.EXTRA:    # (accepted by the filters, next to candidates that are none)
            assert false >= 20, (kind, false)
        elif kind != "random":   # (random is the benign binary case: no condition)
            assert per >= 2, (kind, per)
        if kind in ("stream_in_value", "phase"):
            assert chained > 0, kind
    # the long binary values: fitting lengths throughout the interior of the one value
    for c in B.corpus()["long-alone"]:
        if c.payload == "low" and c.name.startswith("long_"):
            false, chained = B.false_positions(c.stream, c.vals)
            print(f"{c.name}: {false} false positions, {chained} three-link")
            assert false >= 100 and chained > 0, c.name


def _prefixes(case):
    return np.cumsum([0] + [4 + len(v) for v in case.vals])


def test_geometry_lands_where_it_aims():
    C = B.corpus()
    T1 = B.BA_TILE
    by_name = {c.name: c for cases in C.values() for c in cases}
    want = {}
    for k in range(6):
        want[f"straddle_t1-{k}"] = {"prefix": T1 - k}
        want[f"bw_straddle_1k-{k}"] = {"prefix": B.BW_TILE - k, "prefix2": 3 * B.BW_TILE - k}
    for end in (0, 127, 128):
        want[f"value_end_t1+{end}"] = {"prefix": T1 + end - 104, "end": T1 + end}
    for nxt in (172, 173, 176):
        want[f"successor_t1+{nxt}"] = {"prefix": T1 + nxt - 104, "successor": T1 + nxt}
    for n in B.HALO_LENGTHS:
        want[f"halo_{n}_mid"] = {"prefix": 4000}
        want[f"halo_{n}_t1-1"] = {"prefix": T1 - 1}
        want[f"halo_{n}_t1-128"] = {"prefix": T1 - 128}
        want[f"halo_{n}_t1-129"] = {"prefix": T1 - 129}
        want[f"halo_{n}_first"] = {"prefix": 0}
    for name, land in want.items():
        case = by_name[name]
        assert case.land == land, (name, case.land, land)
        pre = _prefixes(case)
        for label, p in land.items():   # recomputed from the values, not from the builder's bookkeeping
            assert p in pre, (name, label, p)
    assert B.BA_STAGE_END - 4 == 172   # the last successor k_ba_tile reads from its stage: r + 4 <= BA_FSTAGE
    for n in B.HALO_LENGTHS:
        for place in B.HALO_PLACES:
            case = by_name[f"halo_{n}_{place}"]
            pre = _prefixes(case)
            k = int(np.searchsorted(pre, case.land["prefix"]))
            assert len(case.vals[k]) == n and sum(len(v) > 30 for v in case.vals) == 1, case.name
            if place == "last":
                assert k == case.count - 1
    for n in B.LONG_LENGTHS:
        for payload in ("text", "low"):
            for among in ("among", "alone"):
                case = by_name[f"long_{n}_{payload}_{among}"]
                assert max(len(v) for v in case.vals) == n and case.short() == (among == "among"), case.describe()
    for n in B.STREAM_SIZES:
        assert len(by_name[f"size_{n}"].stream) == n and len(by_name[f"size_{n}_opt"].stream) == n
    for k in (1, 2, 3):
        assert by_name[f"count_{k}"].count == k


def test_fused_files_stay_short(ba_file):
    """plan_ba_walks (pf_plan.cpp) sends a batch to the multi-kernel walk when one page body exceeds
    BA_SHORT bytes per value; the whole page with its header is the upper bound used here."""
    for fid in FILE_IDS:
        f = ba_file(fid)
        for case, ch in zip(f["cases"], f["chunks"]):
            if case.layout == "c":
                continue
            page = len(ch.dict) if case.where == "dict" else len(ch.pages[-1])
            short = page <= B.BA_SHORT * max(1, case.count)
            if fid not in ("long-alone", "dict-long"):
                assert short, (fid, case.describe(), page)
            elif fid == "dict-long":
                assert short == (case.where == "data"), (fid, case.describe(), page)
    assert any(len(ch.pages[-1]) > B.BA_SHORT * c.count for c, ch in
               zip(ba_file("long-alone")["cases"], ba_file("long-alone")["chunks"]))


def test_stream_start_residues(ba_file):
    f = ba_file("residue")
    seen = {}
    for case, info in zip(f["cases"], f["info"]):
        r = B.stream_residue(info)
        print(f"{case.name}: value section at chunk offset {info['values'][-1][0] - info['offset']} (mod 16: {r})")
        seen.setdefault((case.payload, case.layout), set()).add(r)
    for payload in ("zeros", "text"):
        for lay in ("a", "e"):
            assert seen[(payload, lay)] == set(range(16)), (payload, lay, sorted(seen[(payload, lay)]))
        assert len(seen[(payload, "c")]) == 1


def test_restated_rules_give_the_derived_routes():
    """ba_streams.fused_outcome / multi_kernel_outcome restate the filters of pf_ba.hip; the GPU tests
    hold the route counters to them. Here they must give what the rules say for the cases where that can
    be worked out by hand:
      * text whose values are at most 124 bytes (sv - q <= BA_HALO), wherever the 124-byte value lies:
        accepted on the fused route; one 125-byte value (not the page's last): re-linked;
      * text on the multi-kernel route, values of any length: accepted (k_ba_link links at any distance);
      * stream_in_value: inner chains pass both link levels on either route and in the re-link: walked;
      * empty: m & ~(m >> 1) keeps the last position only, position 0 is not accepted: walked;
      * a complete extra record: one accepted position over the count everywhere: walked;
      * a last value past the halo ends at the stream end, which the chain check lets pass: accepted."""
    by_name = {c.name: c for cases in B.corpus().values() for c in cases}

    def fused(name):
        return B.fused_outcome(by_name[name].stream, by_name[name].count)

    def multi(name):
        return B.multi_kernel_outcome(by_name[name].stream, by_name[name].count)

    assert fused("text_req_a") == "accepted" and multi("text_req_a") == "accepted"
    for place in B.HALO_PLACES:
        for n in B.HALO_LENGTHS:
            want = "accepted" if n <= B.BA_MAX_LINKED or place == "last" else "re-linked"
            assert fused(f"halo_{n}_{place}") == want, (n, place)
            assert multi(f"halo_{n}_{place}") == "accepted", (n, place)
    for n in B.LONG_LENGTHS:
        assert multi(f"long_{n}_text_alone") == "accepted" and multi(f"long_{n}_text_among") == "accepted"
        assert fused(f"long_{n}_text_among") == "re-linked"
    for name in ("stream_in_value_req_a", "empty_req_a", "trail_record"):
        assert fused(name) == "walked" and multi(name) == "walked", name
    for fid, cases in B.corpus().items():
        print(fid, "fused (re-linked, walked)", B.expected_counts(cases, "fused"), "multi-kernel", B.expected_counts(cases, "multi"))
    for kind in B.FAMILIES + B.EXTRA:
        print(f"{kind}: fused {fused(kind + '_req_a')}, multi-kernel {multi(kind + '_req_a')}")
