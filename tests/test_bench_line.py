"""The line bench.py prints must stay machine-readable: ONE compact JSON record under 4 KB with the
contract's keys, ``roofline`` and ``cpu_baseline`` (the round-4 line had grown to 21 KB and the
driver could no longer parse it).  The compaction is exercised on a committed full record without a GPU; one GPU test
runs a plain ``bench.py`` end to end."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

FULL = os.path.join(ROOT, "profiles", "r4_bench_line.json")


@pytest.fixture()
def full():
    return json.load(open(FULL))


def test_compact_line_is_small_and_complete(full):
    rec = bench.compact_record(full)
    line = json.dumps(rec, separators=(",", ":"))
    assert len(line) < 4096 and "\n" not in line
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert key in rec, key
    assert rec["value"] == pytest.approx(full["value"], rel=1e-5)
    assert rec["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)
    assert 0.0 < rec["roofline"]["frac"] <= 1.0
    assert rec["roofline"]["bound"] in ("hbm", "mfma") and rec["roofline"]["unit"] in ("GB/s", "TFLOP/s")
    assert rec["roofline"]["achieved"] / rec["roofline"]["peak"] == pytest.approx(rec["roofline"]["frac"], rel=1e-4)
    assert rec["cpu_baseline"]["value"] > 0 and rec["cpu_baseline"]["cores"] >= 1
    assert rec["config"]["workload"] and "model" not in rec["config"]
    # one number per extra leg
    assert {"tts_ms", "w33_ms", "fp32_ms", "C2_frac", "C3_frac", "C5_frac"} <= set(rec["legs"])


def test_compact_line_never_outgrows_the_limit(full):
    # a record with absurdly many legs still compacts below the limit, keeping the contract's keys
    full["configs"].update({"X%03d" % i: {"ms": 1.0, "mixed_roofline_frac": 0.5} for i in range(400)})
    rec = bench.compact_record(full)
    assert len(json.dumps(rec, separators=(",", ":"))) < bench.COMPACT_LIMIT
    assert "roofline" in rec and "cpu_baseline" in rec and "value" in rec


def test_emit_prints_one_last_line(full, capsys, tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    bench.emit(full)
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and len(out[0]) < 4096
    rec = json.loads(out[0])
    assert rec["roofline"]["frac"] > 0 and rec["cpu_baseline"]["value"] > 0
    assert json.load(open(tmp_path / rec["full_record"]))["value"] == full["value"]


def test_pmc_traffic_lookup_normalises_template_arguments():
    # the executor names a stem kernel with its trailing template arguments at their defaults (12 of 14)
    short = "stem2_kernel<false,false,1,1,2,1,true,0,false,true,false,false>"
    long_ = "stem2_kernel<false, false, 1, 1, 2, 1, true, 0, false, true, false, false, 0, false>"
    assert bench.norm_kernel_name(short) == bench.norm_kernel_name(long_)
    assert bench.norm_kernel_name(short.replace("stem2_", "stem2h_")) == bench.norm_kernel_name(long_.replace("stem2_", "stem2h_"))
    assert bench.norm_kernel_name(short.replace("stem2_", "stem2h_")) != bench.norm_kernel_name(short)
    # the committed counter passes are the round-6 build's: the dominant pair in the fp16 x 2 arithmetic (stem2h_kernel),
    # on specialised waves (the 17th template argument), spelled without blanks by the executor and with them by rocprof
    xm = "stem2h_kernel<false,false,1,1,2,1,true,0,false,true,false,false,0,false,true,false,true>"
    traffic, _ = bench.pmc_traffic_for(bench.TREE, xm)
    assert traffic == pytest.approx(68.7e9, rel=0.01)
    traffic, _ = bench.pmc_traffic_for(bench.TREE, xm.replace(",", ", "))
    assert traffic == pytest.approx(68.7e9, rel=0.01)


def test_no_field_of_the_compact_line_is_cut_by_the_drivers_parser(full):
    """The driver keeps 128 characters of a string field and one level of nesting below ``roofline``:
    every string of the compact record stays under 120 characters, the workload included, and the mixed
    per-step roofline fraction is a flat key next to ``frac``."""
    full = dict(full)
    full["config"] = dict(full["config"], workload="Sycamore n53 m20 amplitude, sliced tree, one slice per step per GPU",
                          network="examples/benchmarks/sycamore_n53_m20_s0_e0_pABCDCDAB.json", width_log2=32, arena_gib=113.0)
    full["roofline"] = dict(full["roofline"], mixed_per_step={"bound_ms": 107.8, "frac": 0.49})
    rec = bench.compact_record(full)

    def strings(x, path=""):
        if isinstance(x, dict):
            for k, v in x.items():
                yield from strings(v, path + "/" + str(k))
        elif isinstance(x, (list, tuple)):
            for i, v in enumerate(x):
                yield from strings(v, path + "/" + str(i))
        elif isinstance(x, str):
            yield path, x

    for path, text in strings(rec):
        assert len(text) <= 120, (path, len(text))
    assert rec["roofline"]["mixed_frac"] == pytest.approx(0.49)
    assert all(not isinstance(v, dict) for v in rec["roofline"].values())
    assert rec["config"]["width_log2"] == 32 and rec["config"]["tree"]


def test_plain_record_keeps_the_contract_without_the_full_legs(full):
    """A plain run (no ``--full``) profiles no slice and runs no CPU leg: its compact line still carries the
    contract's keys, and no empty ``roofline`` stands in for the one it did not measure."""
    plain = {k: v for k, v in full.items() if k not in ("roofline", "precision", "cpu_baseline", "configs")
             and not k.startswith(("time_to_solution", "peak_rate")) and not k.endswith("_arithmetic")}
    rec = bench.compact_record(plain)
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "config"):
        assert key in rec, key
    assert rec["ms_per_step"] == pytest.approx(full["ms_per_step"], rel=1e-5)
    assert not {"roofline", "cpu_baseline", "precision", "legs"} & set(rec)


def test_dump_outputs_writes_the_amplitude_as_real_pairs(tmp_path):
    import numpy as np
    import torch

    result = torch.tensor(1.5 - 0.25j, dtype=torch.complex64)
    bench.dump_outputs(str(tmp_path / "out"), result)
    got = np.load(tmp_path / "out" / "amplitude.npy")
    assert got.dtype == np.float32 and got.shape == (2,)
    assert got.tolist() == [1.5, -0.25]


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_what_they_computed(tmp_path):
    """``bench.py --steps 3 --warmup 1 --dump-outputs DIR``: the line holds the contract's keys and the three timed
    slices, nothing a plain run does not measure, and ``DIR/amplitude.npy`` is the partial amplitude of the run."""
    import subprocess

    import numpy as np

    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in rec, key
    assert rec["steps"] == 3 and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(rec["config"]["flops_per_slice"] / (rec["ms_per_step"] * 1e-3), rel=1e-4)
    assert not {"roofline", "cpu_baseline", "precision", "legs"} & set(rec)
    amp = np.load(out / "amplitude.npy")
    assert amp.dtype == np.float32 and amp.shape == (2,) and np.isfinite(amp).all() and np.abs(amp).max() > 0
    full = json.load(open(os.path.join(ROOT, rec["full_record"])))
    assert amp.tolist() == full["config"]["partial_amplitude"]
    # (the headline tree shares steps over slice groups of 4: three timed slices are one group begun, not four)
    assert full["config"]["slice_groups"]["timed"] == "3 slices in 1 groups"


@pytest.mark.gpu
def test_plain_run_dumps_the_amplitude_the_oracle_computes(tmp_path):
    """A plain run over ALL 64 slices of the Sycamore m10 tree (the bench's seeded synthetic inputs): the dumped amplitude
    is the whole contraction, against the numpy complex128 oracle within the single-precision gate of ``smoke()``."""
    import subprocess

    import numpy as np

    import cotengra_amd as ca
    from oracle import contract_ref as orc

    path = os.path.join(bench.TREES, "sycamore_m10.json")
    tree = ca.tree_from_record(ca.load_network(path))
    assert tree.nslices == 64
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "64", "--warmup", "1",
           "--tree", path, "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    assert json.loads(r.stdout.strip().splitlines()[-1])["steps"] == 64
    re_, im = np.load(out / "amplitude.npy").tolist()
    got = complex(re_, im)
    arrays = ca.make_arrays_from_inputs(tree.inputs, tree.size_dict, seed=42, dtype="complex64", rescale=True)
    ref = complex(orc.contract(tree, [a.astype("complex128") for a in arrays]))
    gate = max(1e-5, 8.0 * abs(complex(orc.contract(tree, arrays)) - ref) / abs(ref))
    assert abs(got - ref) <= gate * abs(ref), (got, ref, abs(got - ref) / abs(ref), gate)
