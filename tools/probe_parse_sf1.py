"""Diagnostic (stamps build: PFLOOR_LIB_PATH=parquet-floor_amd/diag/libpfloor_stamps.so): the Snappy parse
kernels' phase counters (pf_debug_cstamps, CSTAMP slots of pf_snappy_parse.hip) for one lineitem row group
(all 16 columns in one batch): index pass per window (with the successor record's walk: steps, answers, and the
histogram of the bytes past the next window's start that a resolved walk read), chain pass per page.
A library built with -DPF_IDX_EXT=4096 (make variant) shows the histogram beyond the product's extension."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "parquet-floor_amd")]
import pyarrow.parquet as pq  # noqa: E402
from pfloor import _native, datagen  # noqa: E402
from pfloor.decoder import GpuDecoder, decode_file  # noqa: E402

rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1048576
path = os.path.join(ROOT, "gpurun_out", f"probe_lineitem_{rows}.parquet")
if not os.path.exists(path):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    pq.write_table(datagen.lineitem_table(rows, seed=42), path, compression="snappy", row_group_size=1 << 20)
L = _native.lib()
f = L.pf_debug_cstamps
f.argtypes = [C.POINTER(C.c_ulonglong), C.c_int, C.c_int]
N = 40
buf = (C.c_ulonglong * N)()
with GpuDecoder(0) as dec:
    decode_file(path, row_groups=[0], decoder=dec)
    f(buf, N, 1)
    got = decode_file(path, row_groups=[0], decoder=dec)
    f(buf, N, 1)
b = list(buf)
w = max(b[0], 1)
pages = max(b[17], 1)
merged = sum(b[32:40])
print(f"index: windows {b[0]} | per window cycles: whole wave {b[25] / w:.0f} = spec parse {b[1] / w:.0f} + store {b[3] / w:.0f} "
      f"(wave sum {b[26] / w:.0f} of it) + successor record {b[9] / w:.0f} | no-conv {b[2]}")
print(f"record: asked {b[15]} | merge {merged} slow (step cap) {b[5]} none {b[10]} | steps {b[4]} "
      f"({b[4] / max(b[15], 1):.1f} per asked) | bytes needed, mean of merges {b[6] / max(merged, 1):.0f}, "
      "histogram <=32 <=64 <=128 <=256 <=512 <=1024 <=2048 more: " + " ".join(str(x) for x in b[32:40]))
print(f"chain: pages {b[17]} windows {b[18]} | rounds {b[13]} exact parses {b[14]} ({b[16] / max(b[14], 1):.0f} cycles each) "
      f"deep walks {b[11]} ({b[12] / max(b[11], 1):.0f} cycles each) | per page {b[19] / pages:.0f} cycles, max {b[20]}")
print("raw", b, "status", got["_status"])
