"""The reference of the kept-dictionary filter tests agrees with itself, without a GPU: for every batch, window set and
query of tests/dict_filter_cases.py the expected kept result (the ids the chunk was built from, cut and selected, over
the entries it was built from), expanded with numpy, is bit for bit the expanded chunk cut by window_cases.slice_chunk and
compacted by filter_cases.take_rows. The constants the cases are built around are those of the headers."""
import os
import re

import numpy as np
import pytest

import dict_filter_cases as FD
import window_cases as WC

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "parquet-floor_amd", "csrc")


def _const(header, name):
    with open(os.path.join(CSRC, header)) as fh:
        m = re.search(r"constexpr\s+uint32_t\s+" + name + r"\s*=\s*(\d+)\s*;", fh.read())
    assert m, f"{name} not found in {header}"
    return int(m.group(1))


def test_constants_are_the_headers():
    assert FD.SEL_TILE == _const("pf_internal.h", "SEL_TILE")
    assert FD.SELD_TILE == _const("pf_internal.h", "SELD_TILE")
    assert FD.FBLK == _const("pf_page_tables.h", "FBLK")
    for n in (0, 1, 63, 64, 65, 256, 257, FD.SELD_TILE - 1, FD.SELD_TILE, FD.SELD_TILE + 1, 65536, 65537):
        assert n in FD.DICT_SIZES


def test_the_batches_cover_the_stated_shapes():
    """Dictionary sizes of predicate chunks, and rows_selected at every residue of the gather's 16-byte groups."""
    sizes = set()
    for name, b in FD.BATCHES.items():
        if name.startswith("sizes-"):
            specs, _w, qs = b.build(None)
            sizes |= {specs[p[0][0]].n_dict for _l, p in qs}
    assert set(FD.DICT_SIZES) <= sizes, sorted(set(FD.DICT_SIZES) - sizes)
    specs, _w, qs = FD.BATCHES["selected-residues"].build(None)
    exp = [FD.canon(s, s.chunk.expected()) for s in specs]
    got = {len(FD.reference(specs, exp, None, p)[1]) for _l, p in qs}
    assert {k % 16 for k in got} == set(range(16)) and {0, 63, 64, 65, 127, 128, 129, int(exp[0]["num_rows"])} <= got
    assert {1, 2, 4} <= {FD.DC.index_width(s.n_dict) for s in specs if s.kept}


@pytest.mark.parametrize("name", list(FD.BATCHES))
def test_reference_agrees_with_itself(name):
    specs, windows, queries = FD.BATCHES[name].build(None)
    exp = [FD.canon(s, s.chunk.expected()) for s in specs]
    n_kept = 0
    for label, preds in queries:
        rows_in, idx, expanded, kept = FD.reference(specs, exp, windows, preds)
        if preds:
            assert rows_in is not None and (len(idx) == 0 or (idx[-1] < rows_in and (np.diff(idx) > 0).all()))
        for c, s in enumerate(specs):
            assert (kept[c] is not None) == (s.kept and expanded[c] is not None)
            if kept[c] is None:
                continue
            n_kept += 1
            k = kept[c]
            assert len(k["indices"]) == k["num_slots"] and (k["indices"] >= 0).all()
            assert (k["indices"] < max(s.n_dict, 1)).all()
            WC.assert_window_equal(FD.materialized(k, s.ptype), expanded[c], f"{name} / {label} chunk {c}")
            assert FD.materialized(k, s.ptype)["num_chars"] == expanded[c]["num_chars"]
    assert n_kept > 0
