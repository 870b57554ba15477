"""bench.py's command line and --dump-outputs on the host (no GPU): a plain run is the headline only, and what the last timed step
computed is written as float32 .npy files, whole or as a seeded sample that stays the same from run to run and under 64 MB in all."""
import importlib.util
import os
import sys

import numpy as np
import torch

from conftest import REPO


def _bench(argv):
    spec = importlib.util.spec_from_file_location("pv_bench", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    old, sys.argv = sys.argv, ["bench.py", *argv]
    try:
        return mod, mod.parse()
    finally:
        sys.argv = old


def test_plain_run_is_the_headline_only():
    _, args = _bench(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert args.steps == 7 and args.warmup == 2 and not args.full and args.dump_outputs is None
    _, args = _bench(["--full", "--dump-outputs", "out"])
    assert args.full and args.dump_outputs == "out"


def test_dumped_outputs_are_float32_whole_or_a_fixed_sample(tmp_path):
    bench, _ = _bench([])
    logits = torch.randn(2048, 1000)
    grads = [torch.randn(3072, 768), torch.randn(768)]
    arrays = bench.last_step_outputs(logits, grads)
    assert np.array_equal(arrays["logits"], logits.numpy()) and arrays["logits"].dtype == np.float32
    assert arrays["grad_sample"].dtype == np.float32 and arrays["grad_sample"].shape == (1 << 20,)
    assert np.array_equal(arrays["grad_sample"], bench.last_step_outputs(logits, [g.clone() for g in grads])["grad_sample"])
    big = torch.randn(40000, 1000)
    a, b = bench.last_step_outputs(big, grads), bench.last_step_outputs(big.clone(), grads)
    assert a["logits"].shape[1] == 1000 and a["logits"].shape[0] < 40000 and np.array_equal(a["logits"], b["logits"])
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    bench.write_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == ["grad_sample.npy", "logits.npy"]
    assert np.array_equal(np.load(tmp_path / "d" / "logits.npy"), arrays["logits"])
