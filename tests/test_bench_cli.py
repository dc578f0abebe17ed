"""bench.py's command line: a plain run keeps only the timed steps, --full brings the other legs
back, and --dump-outputs writes the last timed step's arrays as float32 / float64 .npy files,
sampled at fixed positions where large, with whole-array checksums beside them.

CPU: the argument handling, and dump_outputs over stand-in decoders (sampling, determinism, size
bound). GPU: one plain run of the smallest workload (config 1, 1,000,000 flat rows) whose dumped
arrays and checksums are compared with the CPU oracle's decode of the same file."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402

LEGS = ("no_cpu_baseline", "no_parity", "no_e2e", "no_pmc", "no_write")


def test_plain_run_has_every_extra_leg_off():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert all(getattr(a, leg) for leg in LEGS)
    a = bench.parse_args(["--full"])
    assert a.full and not any(getattr(a, leg) for leg in LEGS)
    a = bench.parse_args(["--full", "--no-e2e", "--dump-outputs", "somewhere"])
    assert a.no_e2e and not a.no_parity and a.dump_outputs == "somewhere"


class _Col:
    def __init__(self, physical_type, max_def, max_rep):
        self.physical_type, self.max_def, self.max_rep = physical_type, max_def, max_rep


class _PF:
    # INT64 optional, BYTE_ARRAY optional, DOUBLE required, INT32 in an optional list, FLOAT required, BOOLEAN required
    columns = [_Col(2, 1, 0), _Col(6, 1, 0), _Col(5, 0, 0), _Col(1, 2, 1), _Col(4, 0, 0), _Col(0, 0, 0)]


class _Batch:
    items = [(3, c, 0, 0, 0) for c in range(len(_PF.columns))]


class _Dec:
    """Stands in for a GpuDecoder whose last batch is resident: fetch() as GpuDecoder.fetch returns it."""

    def __init__(self, seed, n=5001):
        self.seed, self.n = seed, n

    def fetch(self, i, physical_type, max_def, max_rep):
        rng = np.random.default_rng([self.seed, i])
        n, rows = self.n, self.n // 3
        g = {"status": 0, "num_slots": n, "num_rows": rows}
        if physical_type == 6:
            lens = rng.integers(0, 9, n)
            g["offsets"] = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
            g["chars"] = rng.integers(32, 127, int(lens.sum())).astype(np.uint8)
        elif physical_type in (4, 5):
            g["values"] = rng.standard_normal(n).astype(bench._VALUE_DTYPE[physical_type]).view(np.uint8)
        elif physical_type == 0:
            g["values"] = rng.integers(0, 2, n).astype(np.uint8)
        else:
            g["values"] = rng.integers(-2**31, 2**31, n).astype(bench._VALUE_DTYPE[physical_type]).view(np.uint8)
        if max_def > 0:
            g["validity"] = rng.integers(0, 256, (n + 7) // 8).astype(np.uint8)
        if max_rep == 1:
            g["list_offsets"] = np.linspace(0, n, rows + 1).astype(np.int32)
            g["list_validity"] = rng.integers(0, 256, (rows + 7) // 8).astype(np.uint8)
        if max_rep > 0:
            g["def_levels"] = rng.integers(0, 3, n).astype(np.uint8)
            g["rep_levels"] = rng.integers(0, 2, n).astype(np.uint8)
        return g


def _typed(g, name, col):
    """The array `name` of fetched chunk g as the numbers a caller reads from it."""
    a = np.asarray(g[name])
    if name == "values" and col.physical_type in bench._VALUE_DTYPE:
        return a.view(np.uint8).view(bench._VALUE_DTYPE[col.physical_type])
    if name in ("validity", "list_validity"):
        return np.unpackbits(a.view(np.uint8), bitorder="little")[:g["num_slots"] if name == "validity" else g["num_rows"]]
    return a


def _checksum(a):
    return [float(a.size)] + [float(a[::st].sum(dtype=np.float64)) for st in (1, 2, 3)]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _assert_dumped(got, exp, key, col):
    """got: the dumped array `key`; exp: the whole array it was taken from, as numbers."""
    assert got.dtype in (np.float32, np.float64), key
    s, i, _rg, _c, name = key.split("_", 4)
    whole = got.size == exp.size
    if not whole:                # sampled: the values at the fixed positions
        assert 0 < got.size < exp.size, key
        k = bench._chunk_array_names(col).index(name)
        exp = exp[bench.sample_positions(int(s[1:]), int(i[1:]), k, exp.size, got.size)]
    assert np.array_equal(got, exp.astype(got.dtype)), key
    assert np.array_equal(got.astype(exp.dtype), exp), key   # the float type holds these values exactly
    return whole


@pytest.mark.parametrize("budget", [1 << 30, 40_000])   # everything whole / every long array sampled
def test_dump_outputs_whole_and_sampled(tmp_path, monkeypatch, budget):
    monkeypatch.setattr(bench, "DUMP_BUDGET", budget)
    decs = [_Dec(1), _Dec(2)]
    n = bench.dump_outputs(str(tmp_path / "a"), _PF, decs, [_Batch, _Batch])
    assert n == 2 * 14                                   # 2, 3, 1, 6, 1, 1 arrays per stream
    assert bench.dump_outputs(str(tmp_path / "b"), _PF, decs, [_Batch, _Batch]) == n
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert list(a) == list(b) and len(a) == n + 1
    names = [k for k in a if k != "checksums"]
    assert a["checksums"].shape == (n, 4) and a["checksums"].dtype == np.float64
    payload = 0
    for row, key in zip(a["checksums"], names):
        got = a[key]
        assert got.tobytes() == b[key].tobytes(), key            # same inputs, same files
        payload += got.nbytes
        s, i, rg, c, name = key.split("_", 4)
        assert rg == "rg3"
        col = _PF.columns[int(c[1:])]
        exp = _typed(decs[int(s[1:])].fetch(int(i[1:]), col.physical_type, col.max_def, col.max_rep), name, col)
        assert list(row) == _checksum(exp), key                   # over the whole array, sampled or not
        whole = _assert_dumped(got, exp, key, col)
        assert whole == (budget == 1 << 30), key
    assert payload <= budget


def test_dump_outputs_refuses_a_failed_chunk(tmp_path):
    class Failed(_Dec):
        def fetch(self, *a):
            return {"status": 5}
    with pytest.raises(RuntimeError, match="status 5"):
        bench.dump_outputs(str(tmp_path), _PF, [Failed(1)], [_Batch])


@pytest.mark.gpu
def test_plain_bench_run_dumps_what_it_decoded(oracle, tmp_path_factory):
    """One plain run and nothing else: the line has the headline fields and none of --full's, --steps
    is the number of timed steps, and every dumped array (or, where sampled, its whole-array checksum)
    equals the oracle's decode of the file the run wrote."""
    d = tmp_path_factory.mktemp("bench")
    dump = str(d / "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--warmup-s", "0", "--workload", "flat", "--data-dir", str(d), "--dump-outputs", dump],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "decoded GB/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u8" and line["steps"] == 3 and line["n_gpus"] == 1
    assert line["warmup_policy"]["passes_run"] == 1
    assert line["ms_per_step"] > 0
    per_step = line["config"]["decoded_bytes_per_step"]
    # the line rounds ms_per_step to 1e-4 ms: 5e-5 / 0.025 ms (a step far shorter than this one) = 2e-3
    assert line["value"] == pytest.approx(per_step / (line["ms_per_step"] * 1e-3) / 1e9, rel=2e-3)
    for k in ("parity", "e2e", "write", "cpu_baseline", "roofline", "stage_ms", "pmc_traffic_per_launch"):
        assert k not in line, k

    got = _load(dump)
    names = [k for k in got if k != "checksums"]
    assert got["checksums"].shape == (len(names), 4)
    assert sum(os.path.getsize(os.path.join(dump, f)) for f in os.listdir(dump)) <= 64 * 10**6
    path = bench.input_path(bench.parse_args(["--workload", "flat", "--data-dir", str(d)]))
    seen, decoded = set(), 0
    with oracle.open(path) as of:
        cols = [_Col(of.schema(c)["type"], of.schema(c)["max_def"], of.schema(c)["max_rep"]) for c in range(of.num_columns)]
        cache = {}
        for row, key in zip(got["checksums"], names):
            _s, _i, rg, c, name = key.split("_", 4)
            rg, c = int(rg[2:]), int(c[1:])
            if (rg, c) not in cache:
                cache[(rg, c)] = of.decode(rg, c)
                assert cache[(rg, c)]["status"] == 0
            exp = _typed(cache[(rg, c)], name, cols[c])
            assert (rg, c, name) not in seen
            seen.add((rg, c, name))
            assert list(row) == _checksum(exp), key
            _assert_dumped(got[key], exp, key, cols[c])
            decoded += np.asarray(cache[(rg, c)][name]).nbytes
        # every chunk of the file was decoded by exactly one stream in the last step, and the dump holds all of them
        assert {(rg, c) for rg, c, _ in seen} == {(rg, c) for rg in range(of.num_row_groups) for c in range(of.num_columns)}
    assert decoded == per_step
