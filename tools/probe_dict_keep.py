"""Measurements of the kept-dictionary decode on bench.py's SF1 file (lineitem, 6,001,215 rows):

  python tools/probe_dict_keep.py bytes            D2H bytes of row group 0, kept against expanded: pf_batch_bytes and
                                                   per column (exact counts from pf_column_info / pf_dict_info)
  python tools/probe_dict_keep.py flat             stage_ms.flat of row group 0 (device-resident input, median of 20),
                                                   kept against expanded: all 16 columns, and the eligible columns alone
                                                   (k_flat_ids + k_dict_offsets + k_dict_pack against the flat kernels
                                                   that expand the same chunks)
  python tools/probe_dict_keep.py e2e --mode kept|expanded
                                                   one pass over the file: every row group uploaded from pinned memory,
                                                   decoded, and brought back by pf_copy_batch_async into pinned memory
                                                   (two contexts on one stream, the next decode enqueued before the
                                                   copy). Prints ms per pass (best of --passes) and the bytes that came back.
PFLOOR_LIB_PATH selects the library (a build of the parent commit for the expanding baseline: --mode expanded uses
only calls it has)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "parquet-floor_amd")]
import bench  # noqa: E402
from pfloor import _native  # noqa: E402
from pfloor.decoder import GpuDecoder, ParquetFile, PinnedBuffer  # noqa: E402


def sf1():
    return bench.make_input(argparse.Namespace(workload="sf1", data_dir=os.environ.get("PF_BENCH_DIR", "/tmp/pfloor_bench"), pool=100000))


class Batch:
    """The chunks of `cols` of one row group in a pinned buffer."""

    def __init__(self, pf, dec, rg, cols):
        items, total = pf.plan([rg], cols)
        self.nbytes = max(total, 1)
        self.host = PinnedBuffer(dec.h, self.nbytes)
        for _rg, _col, s, n, off in items:
            if n:
                pf.read_into(s, n, self.host.ptr.value + off)
        self.descs = [pf.chunk_desc(r, c, off) for r, c, _s, _n, off in items]
        self.arr = (_native.ChunkDesc * max(1, len(self.descs)))(*self.descs)
        self.cols = cols


def batch_bytes(dec):
    n = C.c_size_t()
    _native.check(_native.lib().pf_batch_bytes(dec.h, C.byref(n)), dec.h, "pf_batch_bytes")
    return n.value


def chunk_bytes(dec, i):
    """Bytes of chunk i's arrays as the batch copy carries them (indices or values, validity, offsets, chars, dictionary)."""
    ci = dec.info(i)
    n = ci.num_slots * ci.width + (4 * (ci.num_slots + 1) if ci.d_offsets else 0) + ci.num_chars
    n += (ci.num_slots + 7) // 8 if ci.d_validity else 0
    if hasattr(_native.lib(), "pf_dict_info_get"):
        di = dec.dict_info(i)
        if di.kept:
            n += di.n_entries * di.width + (4 * (di.n_entries + 1) if di.d_offsets else 0) + di.num_chars
    return n


def cmd_bytes(path):
    with ParquetFile(path) as pf, GpuDecoder(0) as dec:
        cols = list(range(pf.num_columns))
        b = Batch(pf, dec, 0, cols)
        rows = {}
        for tag, keep in (("expanded", None), ("kept", [True] * len(cols))):
            dec.decode(b.arr, b.host.ptr.value, b.nbytes, keep=keep) if keep else dec.decode(b.arr, b.host.ptr.value, b.nbytes)
            assert dec.wait() == 0, dec.error()
            rows[tag] = (batch_bytes(dec), [chunk_bytes(dec, i) for i in range(len(cols))],
                         [dec.dict_info(i).kept for i in range(len(cols))])
        print(f"row group 0 ({pf.row_group_rows(0)} rows): pf_batch_bytes expanded {rows['expanded'][0]}, kept {rows['kept'][0]} "
              f"({rows['kept'][0] / rows['expanded'][0]:.3f})")
        for i, c in enumerate(cols):
            e, k = rows["expanded"][1][i], rows["kept"][1][i]
            print(f"  {pf.columns[c].path[0]:16s} expanded {e:10d}  kept {k:10d}  {'kept' if rows['kept'][2][i] else 'as ever':8s} {k / max(e, 1):.3f}")


def cmd_flat(path, reps=20):
    with ParquetFile(path) as pf, GpuDecoder(0) as dec:
        every = list(range(pf.num_columns))
        b = Batch(pf, dec, 0, every)
        dec.decode(b.arr, b.host.ptr.value, b.nbytes, keep=[True] * len(every))
        assert dec.wait() == 0, dec.error()
        eligible = [c for i, c in enumerate(every) if dec.dict_info(i).kept]
        for label, cols in (("all columns", every), ("eligible columns", eligible)):
            bb = Batch(pf, dec, 0, cols)
            d = C.c_void_p()
            L = _native.lib()
            _native.check(L.pf_device_alloc(dec.h, bb.nbytes, C.byref(d)), dec.h, "pf_device_alloc")
            _native.check(L.pf_memcpy_h2d(dec.h, d, bb.host.ptr, bb.nbytes), dec.h, "h2d")
            for tag, keep in (("expanded", None), ("kept", [True] * len(cols))):
                flat, total = [], []
                for _ in range(reps + 3):
                    dec.decode(bb.arr, d.value, bb.nbytes, on_device=True, keep=keep)
                    assert dec.wait() == 0, dec.error()
                    t = dec.timing()
                    flat.append(t["flat"])
                    total.append(sum(v for k, v in t.items() if k != "h2d"))
                flat, total = flat[3:], total[3:]
                print(f"{label:17s} ({len(cols):2d} chunks) {tag:8s}: stage_ms.flat median {statistics.median(flat):.4f} "
                      f"(min {min(flat):.4f}, max {max(flat):.4f}); all stages {statistics.median(total):.4f} ms")
            L.pf_device_free(dec.h, d)


def cmd_e2e(path, mode, passes):
    L = _native.lib()
    with ParquetFile(path) as pf:
        a = GpuDecoder(0)
        decs = [a, GpuDecoder(share=a)]
        for d in decs:
            d.set_timing(False)
        cols = list(range(pf.num_columns))
        batches = [Batch(pf, decs[0], rg, cols) for rg in range(pf.num_row_groups)]
        keep = [True] * len(cols) if mode == "kept" else None
        outs = [None, None]

        def enqueue(i):
            d, b = decs[i % 2], batches[i]
            if keep:
                d.decode(b.arr, b.host.ptr.value, b.nbytes, keep=keep)
            else:
                d.decode(b.arr, b.host.ptr.value, b.nbytes)

        def one_pass():
            got = 0
            enqueue(0)
            for i in range(len(batches)):
                d = decs[i % 2]
                assert d.wait() == 0, d.error()
                if i + 1 < len(batches):
                    _native.check(L.pf_sync(decs[(i + 1) % 2].h), decs[(i + 1) % 2].h, "pf_sync")   # its last copy has left
                    enqueue(i + 1)
                n = batch_bytes(d)
                if outs[i % 2] is None or outs[i % 2].nbytes < n:
                    outs[i % 2] = PinnedBuffer(d.h, n + n // 8)
                _native.check(L.pf_copy_batch_async(d.h, outs[i % 2].ptr, outs[i % 2].nbytes), d.h, "pf_copy_batch_async")
                got += n
            for d in decs:
                _native.check(L.pf_sync(d.h), d.h, "pf_sync")
            return got
        one_pass()
        one_pass()
        times = []
        for _ in range(passes):
            t0 = time.perf_counter()
            got = one_pass()
            times.append((time.perf_counter() - t0) * 1e3)
        print(json.dumps({"mode": mode, "lib": os.path.basename(_native.LIB_PATH), "ms_per_pass": round(min(times), 3),
                          "ms_all": [round(t, 3) for t in times], "d2h_bytes": got, "row_groups": len(batches)}))
        for d in reversed(decs):
            d.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("bytes", "flat", "e2e"))
    ap.add_argument("--mode", choices=("kept", "expanded"), default="kept")
    ap.add_argument("--passes", type=int, default=10)
    args = ap.parse_args()
    p = sf1()
    if args.what == "bytes":
        cmd_bytes(p)
    elif args.what == "flat":
        cmd_flat(p)
    else:
        cmd_e2e(p, args.mode, args.passes)
