"""The PLAIN BYTE_ARRAY value walk on the stream corpus of tests/ba_streams.py: binary payloads full of
false candidates, and text whose one interesting prefix lands on a chosen byte of the tile geometry.

Every file is decoded three times: by the product library (which picks the fused k_ba_tile walk or, for
the files holding a page above BA_SHORT bytes per value, the multi-kernel one), by the diagnostics build
with its default switches (for the route counters) and by the diagnostics build with PF_BA_FUSED=0
(k_ba_cand / k_ba_link x 2 / k_ba_count / k_ba_verify, which fail straight to binary_walk_wg). Every
chunk must be bit-exact with the construction: offsets, chars, validity, list arrays; a damaged stream
gets the oracle's verdict (test_ba_streams.py), next to chunks that stay bit-exact.

pf_debug_ba_counts gives {jobs re-linked by ba_relink_wg, jobs walked by binary_walk_wg} per decode.
test_route_pins decodes single cases and holds the counters to what the walk's rules say."""
import ctypes as C
import os

import pytest

import ba_streams as B
from golden_util import assert_chunk_equal
from test_ba_streams import FILE_IDS, ba_dir, ba_file  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

# a data page / a dictionary page above BA_SHORT bytes per value: the library itself leaves the fused walk
# for the batch's data pages (ba_short_data false) / dictionary pages (ba_short_dict false, data pages fused)
DATA_MULTI_FILE, DICT_MULTI_FILE = "long-alone", "dict-long"


@pytest.fixture(scope="module")
def decoder():
    from pfloor.decoder import GpuDecoder
    d = GpuDecoder(0)
    yield d
    d.close()


def _ba_counts(reset=True):
    """(re-linked, walked) since the last reset; diagnostics build only (call inside switches())."""
    from pfloor import _native
    f = _native.lib().pf_debug_ba_counts
    f.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    buf = (C.c_ulonglong * 2)()
    assert f(buf, 1 if reset else 0) == 0
    return int(buf[0]), int(buf[1])


def _counted(path, dec):
    from pfloor.decoder import decode_file
    _ba_counts()
    got = decode_file(path, decoder=dec)
    return got, _ba_counts()


def _check(got, f, fid, tag):
    """Every chunk against the construction, or against the oracle's verdict where it rejects the stream."""
    rejected = 0
    for c, (case, exp) in enumerate(zip(f["cases"], f["expected"])):
        g = got[(0, c)]
        where = f"{fid} [{tag}] {case.describe()}"
        if f["verdict"][c] != 0:
            assert g["status"] != 0, f"{where}: the oracle rejects this stream ({f['verdict'][c]}), the GPU reports success"
            rejected += 1
            continue
        assert g["status"] == 0, f"{where}: status {g['status']} on a stream the oracle reads ({got['_error']})"
        assert_chunk_equal(g, exp, where)
    if rejected == 0:
        assert got["_status"] == 0, (fid, tag, got["_error"])
    return rejected


@pytest.mark.parametrize("fid", FILE_IDS)
def test_gpu_corpus(decoder, ba_file, switches, fid):
    from pfloor.decoder import GpuDecoder, decode_file
    f = ba_file(fid)
    got = decode_file(f["path"], decoder=decoder)
    n_rej = _check(got, f, fid, "product library")
    assert n_rej == sum(v != 0 for v in f["verdict"])
    if fid == "damaged":   # the same decoder reads a clean file afterwards
        clean = ba_file("families-req")
        _check(decode_file(clean["path"], decoder=decoder), clean, "families-req", "product library, after the damaged file")
    for env, tag in (({}, "diagnostics build"), ({"PF_BA_FUSED": 0}, "diagnostics build PF_BA_FUSED=0")):
        with switches(**env), GpuDecoder(0) as d:
            got, counts = _counted(f["path"], d)
        print(f"{fid} [{tag}]: {len(f['cases'])} chunks, re-linked {counts[0]}, walked {counts[1]}")
        _check(got, f, fid, f"{tag}, re-linked {counts[0]} walked {counts[1]}")
        # the route every job takes follows from the walk's rules (ba_streams.fused_outcome /
        # multi_kernel_outcome restate them): a filter that gives up on a chain it should accept, or
        # accepts one it should not, moves these counters even where the exact walk hides it from the values
        fused = [c for c in f["cases"] if not env and (c.where == "data" if fid == DICT_MULTI_FILE else fid != DATA_MULTI_FILE)]
        multi = [c for c in f["cases"] if not any(c is x for x in fused)]
        want = tuple(a + b for a, b in zip(B.expected_counts(fused, "fused"), B.expected_counts(multi, "multi")))
        assert counts == want, f"{fid} [{tag}]: re-linked, walked {counts}, by the rules {want}"


def _single(case, oracle, ba_dir):
    data, _info, _chunks, (exp,) = B.build([case], oracle.snappy_compress)
    path = os.path.join(ba_dir, f"single_{case.name}.parquet")
    if not os.path.exists(path):
        with open(path, "wb") as fh:
            fh.write(data)
    return path, exp


def _outcome(counts):
    return "walked" if counts[1] else "re-linked" if counts[0] else "accepted"


def test_route_pins(oracle, ba_dir, switches):
    """One case per decode, so the counters speak of that case's one walk job. The expected counters
    follow from the rules of the walk (pf_ba.hip), not from a run:

    fused (k_ba_tile, then k_ba_fallback):
      * text of values up to 124 bytes, the 124-byte value at every listed position: every successor is
        within BA_HALO of its prefix, text has no other candidates -> accepted: (0, 0);
      * one 125-byte value among them (not the page's last): sv - q = 129 > BA_HALO, the chain check
        rejects the tile (BA_RELINK) and ba_relink_wg links at any distance -> (1, 0);
      * stream_in_value: the inner chains pass both link levels, and ba_relink_wg accepts by the same
        rule, so the count is wrong there too and only the exact walk is right -> walked >= 1;
      * empty: every position is plausible, m & ~(m >> 1) keeps only the last one, position 0 is not
        accepted -> walked >= 1;
      * one complete extra record after the last value: one accepted position over the count, in the
        tiles and in the re-link -> re-linked + walked >= 1, and the page is read.
    multi-kernel (PF_BA_FUSED=0):
      * text, short values or values up to 20,000 bytes: k_ba_link follows a successor at any
        distance -> (0, 0)."""
    from pfloor.decoder import GpuDecoder
    by_name = {c.name: c for cases in B.corpus().values() for c in cases}
    seen = {"fused": {}, "multi": {}}

    def run(d, route, case):
        path, exp = _single(case, oracle, ba_dir)
        got, counts = _counted(path, d)
        print(f"{route}: {case.describe()}: re-linked {counts[0]}, walked {counts[1]}")
        label = f"[{route}, re-linked {counts[0]} walked {counts[1]}] {case.describe()}"
        assert got[(0, 0)]["status"] == 0 and got["_status"] == 0, f"{label}: {got['_error']}"
        assert_chunk_equal(got[(0, 0)], exp, label)
        seen[route][case.name] = _outcome(counts)
        model = (B.fused_outcome if route == "fused" else B.multi_kernel_outcome)(case.stream, case.count)
        assert _outcome(counts) == model, f"{label}: by the rules this job is {model}"
        return counts, label

    with switches(), GpuDecoder(0) as d:
        for name in ["text_req_a"] + [f"halo_124_{p}" for p in B.HALO_PLACES]:
            counts, label = run(d, "fused", by_name[name])
            assert counts == (0, 0), label
        counts, label = run(d, "fused", by_name["halo_125_mid"])
        assert counts == (1, 0), label
        for name in ("stream_in_value_req_a", "empty_req_a"):
            counts, label = run(d, "fused", by_name[name])
            assert counts[1] >= 1, label
        counts, label = run(d, "fused", by_name["trail_record"])
        assert counts[0] + counts[1] >= 1, label
        for kind in B.FAMILIES + B.EXTRA:   # (held to the restated rules in run(), and counted in the coverage below)
            run(d, "fused", by_name[f"{kind}_req_a"])
    with switches(PF_BA_FUSED=0), GpuDecoder(0) as d:
        for name in ["text_req_a"] + [f"long_{n}_text_alone" for n in B.LONG_LENGTHS] + [f"long_{n}_text_among" for n in B.LONG_LENGTHS]:
            counts, label = run(d, "multi", by_name[name])
            assert counts == (0, 0), label
        for kind in B.FAMILIES + B.EXTRA:
            run(d, "multi", by_name[f"{kind}_req_a"])
    for route in seen:
        print(route, {o: sorted(n for n, x in seen[route].items() if x == o) for o in ("accepted", "re-linked", "walked")})
    assert set(seen["fused"].values()) == {"accepted", "re-linked", "walked"}, seen["fused"]
    assert {"accepted", "walked"} <= set(seen["multi"].values()), seen["multi"]
