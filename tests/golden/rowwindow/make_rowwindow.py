"""Fixtures of the row-window tests: pages aligned to rows at irregular edges (no multiple of 8), which the GPU
writer's page_rows never produces. pyarrow 25, seeded; run from this directory: python make_rowwindow.py

3,000 rows: `key` INT64 REQUIRED ascending (128-row pages), `s` OPTIONAL dictionary string (200 words, ~30 % nulls, some empty),
`l` list<int32> with empty lists, null lists and null elements. DataPage v2, 1 KiB pages, page index written; one file
Snappy, one uncompressed. rw_keys.parquet holds the key orders candidate_rows is tested on: `rev` INT64 descending,
`shuf` INT32 shuffled (negative values too), `name` string ascending, `opt` INT32 OPTIONAL ascending with nulls. The script asserts that the v2 num_rows prefix sums equal the OffsetIndex first_row_index,
which the indexed read path relies on."""
import os
import sys

import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq

HERE = os.path.dirname(os.path.abspath(__file__))
ROWS = 3000


def table():
    rng = np.random.default_rng(20251020)
    key = np.cumsum(rng.integers(1, 4, ROWS)).astype(np.int64) + 1000
    words = ["", "a", "bb", "delta", "row-window", "MI355X", "parquet", "x" * 23] + [f"w{i:03d}" for i in range(192)]
    s = [None if rng.random() < 0.3 else words[int(rng.integers(0, len(words)))] for _ in range(ROWS)]
    lists = []
    for _ in range(ROWS):
        u = rng.random()
        if u < 0.12:
            lists.append(None)
        elif u < 0.27:
            lists.append([])
        else:
            n = int(rng.integers(1, 7))
            lists.append([None if rng.random() < 0.15 else int(rng.integers(-1000, 1000)) for _ in range(n)])
    return pa.table({"key": pa.array(key, pa.int64()), "s": pa.array(s, pa.string()),
                     "l": pa.array(lists, pa.list_(pa.int32()))},
                    schema=pa.schema([pa.field("key", pa.int64(), nullable=False), pa.field("s", pa.string()),
                                      pa.field("l", pa.list_(pa.int32()))]))


def keys_table():
    rng = np.random.default_rng(7)
    rev = (np.cumsum(rng.integers(1, 4, ROWS)).astype(np.int64) + 1000)[::-1].copy()
    shuf = rng.permutation(ROWS).astype(np.int32) - 1500
    name = sorted(("n%05d-" % int(v)) + "y" * int(rng.integers(0, 30)) for v in rng.integers(0, 50000, ROWS))
    opt = [None if (i // 300) % 3 == 1 or rng.random() < 0.1 else int(i // 7) for i in range(ROWS)]
    return pa.table({"rev": pa.array(rev, pa.int64()), "shuf": pa.array(shuf, pa.int32()),
                     "name": pa.array(name, pa.string()), "opt": pa.array(opt, pa.int32())},
                    schema=pa.schema([pa.field("rev", pa.int64(), nullable=False), pa.field("shuf", pa.int32(), nullable=False),
                                      pa.field("name", pa.string(), nullable=False), pa.field("opt", pa.int32())]))


def check(path):
    sys.path.insert(0, os.path.join(HERE, "..", "..", "..", "parquet-floor_amd"))
    from pfloor.decoder import ParquetFile
    with ParquetFile(path) as f:
        for col in range(f.num_columns):
            oi = f.page_index(0, col)["offset_index"]
            assert oi is not None, "no OffsetIndex"
            d = f.chunk_desc(0, col, 0)
            data = [d.pages[i] for i in range(d.n_pages) if d.pages[i].page_type == 3]
            assert len(data) == len(oi) and len(data) == d.n_pages - (d.pages[0].page_type == 2)
            first = np.concatenate([[0], np.cumsum([p.num_rows for p in data])])
            assert list(first[:-1]) == [r for _o, _s, r in oi], "v2 num_rows prefix sums != first_row_index"
            assert first[-1] == ROWS
            print(os.path.basename(path), f.columns[col].path, "first rows", list(first[:6]), "...", len(oi), "pages")


if __name__ == "__main__":
    t = table()
    for name, codec in (("rw_snappy.parquet", "snappy"), ("rw_none.parquet", "none")):
        out = os.path.join(HERE, name)
        pq.write_table(t, out, compression=codec, write_page_index=True, data_page_version="2.0", data_page_size=1024,
                       write_batch_size=64, use_dictionary=["s"], write_statistics=True, row_group_size=ROWS)
        assert os.path.getsize(out) < 64 << 10, os.path.getsize(out)
        check(out)
    out = os.path.join(HERE, "rw_keys.parquet")
    pq.write_table(keys_table(), out, compression="snappy", write_page_index=True, data_page_version="2.0",
                   data_page_size=1024, write_batch_size=64, use_dictionary=False, write_statistics=True,
                   row_group_size=ROWS)
    assert os.path.getsize(out) < 64 << 10, os.path.getsize(out)
    check(out)
