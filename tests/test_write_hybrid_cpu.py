"""RLE / bit-packed hybrid write path (PF_ENCODE_HYBRID_RUNS), host side (no GPU).

The expected bytes of the GPU tests (test_gpu_write_hybrid.py) are the streams of hybrid_cases.encode, a
literal restatement of parquet-mr's RunLengthBitPackingHybridEncoder. Here every case of
tests/hybrid_cases.py is wrapped in hand-built v2 pages, with that stream as the page's values section,
and read back to its inputs by the CPU oracle and by pyarrow: two readers that share no code with the
encoder. pagekit builds the level streams of those pages itself, so the reference's level streams are
checked through hybrid_cases' own decoder. Two fixed points are pinned: the four bytes of 20,000 equal
levels, and the case on which pagekit's "mr" style is not parquet-mr's encoder."""
import numpy as np
import pytest

import hybrid_cases as HC
import pagekit as K
from golden_util import assert_chunk_equal


@pytest.mark.parametrize("fid", HC.FILE_IDS)
def test_expected_streams_read_by_oracle_and_pyarrow(oracle, tmp_path, fid):
    pq = pytest.importorskip("pyarrow.parquet")
    rows, cases = HC.file_cases(fid)
    chunks = []
    for case in cases:
        ch = K.Chunk(case.name, case.ptype, optional=case.optional, layout=K.LAYOUTS["e"])
        if case.encoding == K.RLE_DICTIONARY:
            ch.set_dictionary(case.pagekit_vals(case.dictionary))
        for present, vals, ids in case.pages():
            stream = case.values_stream(ids)
            ch.add_page(case.encoding, stream, present=present, vals=case.pagekit_vals(vals))
            # the reference's own streams decode to what went in, to the last byte
            skip = 4 if case.ptype == K.BOOLEAN else 1
            if case.encoding != K.PLAIN:
                assert HC.decode(stream[skip:], case.bw, len(ids)) == [int(x) for x in ids], (fid, case.name)
            if case.optional:
                lv = case.levels_stream(present)
                assert HC.decode(lv, 1, len(present)) == [int(x) for x in present], (fid, case.name)
        chunks.append(ch)
    data, _info = K.build_file(chunks, rows)
    path = str(tmp_path / f"{fid}.parquet")
    with open(path, "wb") as f:
        f.write(data)
    with oracle.open(path) as of:
        assert of.num_columns == len(cases)
        for c, case in enumerate(cases):
            o = of.decode(0, c)
            assert o["status"] == 0, (fid, case.name, o["error"])
            assert_chunk_equal(o, case.expected(), f"{fid} {case.name} [oracle]")
    if rows == 0:
        return
    t = pq.ParquetFile(path).read_row_group(0)
    assert t.num_rows == rows
    for case in cases:
        assert t.column(case.name).to_pylist() == case.pylist(), f"{fid} {case.name} [pyarrow]"


def test_all_present_levels_are_four_bytes():
    assert HC.encode([1] * 20000, 1) == bytes.fromhex("c0b80201")


def test_width_of_dictionary():
    assert [HC.id_width(d) for d in (1, 2, 3, 100, 256, 257, 65536, 65537)] == [0, 1, 2, 7, 8, 9, 16, 17]
    assert HC.encode([0] * 1000, 0) == bytes([0xd0, 0x0f])          # one RLE run, no value bytes


def test_pagekit_mr_style_is_not_this_encoder():
    """A group that ate the head of a repeat: parquet-mr keeps the header open (one run of 2 groups), pagekit's
    "mr" style starts a new one (two runs of 1 group). Both decode to the same values."""
    v = [0] + [1] * 10
    ref, kit = HC.encode(v, 1), K.hybrid(v, 1, "mr")
    assert ref == bytes([0x05, 0xfe, 0x07])
    assert kit == bytes([0x03, 0xfe, 0x03, 0x07])
    assert ref != kit
    assert HC.decode(ref, 1, 11) == v and HC.decode(kit, 1, 11) == v


def test_first_occurrence_ids():
    ids, d = HC.first_occurrence_ids(np.array([7, 3, 7, 9, 3, 3], np.int32))
    assert ids.tolist() == [0, 1, 0, 2, 1, 1] and d.tolist() == [7, 3, 9]
