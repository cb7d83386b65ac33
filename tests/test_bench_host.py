"""Host-side logic of bench.py that needs no GPU: usable-core detection of the CPU baseline and the argument surface
the driver relies on."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def test_usable_cores_respects_affinity_and_is_positive():
    import bench
    n = bench.usable_cores()
    assert 1 <= n <= (os.cpu_count() or 1)
    try:
        assert n <= len(os.sched_getaffinity(0))
    except AttributeError:
        pass


def test_driver_flags_and_defaults(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    assert (a.gpus, a.batch, a.spec, a.dtype, a.global_batch) == (1, 256, "vitb16", "bf16", 0)
    assert a.steps >= 5 and a.warmup >= 1 and not a.full_loss and a.cpu_baseline_worker == 0
    assert not a.full and a.dump_outputs is None          # a plain run times the headline only
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "8", "--steps", "20", "--warmup", "5", "--global-batch", "2048",
                                      "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup, a.global_batch, a.full, a.dump_outputs) == (8, 20, 5, 2048, True, "out")
    # per-pair work table of the roofline's step fraction
    assert abs(bench.GF_PER_PAIR[("vitb16", False)] - 109.675) < 1e-3


def test_dump_outputs_writes_loss_and_seeded_gradient_samples(tmp_path):
    """--dump-outputs: loss (float64) and one float32 file per parameter gradient; a gradient above the per-tensor share
    is a fixed sample, the same on every call; all files together stay within the 64 MB the option promises."""
    import numpy as np
    import torch
    import bench
    model = torch.nn.Sequential(torch.nn.Linear(300, 400), torch.nn.Linear(400, 3))
    model[1].weight.requires_grad_(False)
    loss = model(torch.randn(5, 300)).square().sum()
    loss.backward()
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), loss, model)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grad.0.bias.npy", "grad.0.weight.npy", "grad.1.bias.npy", "loss.npy"]
    lo = np.load(tmp_path / "a" / "loss.npy")
    assert lo.dtype == np.float64 and lo.shape == () and abs(float(lo) - float(loss)) < 1e-6 * abs(float(loss))
    w = np.load(tmp_path / "a" / "grad.0.weight.npy")
    assert w.dtype == np.float32 and w.shape == (bench.DUMP_SAMPLE,)        # 120000 elements: sampled
    assert np.isin(w, model[0].weight.grad.numpy().reshape(-1)).all()
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "grad.0.bias.npy"), model[0].bias.grad.numpy())
    for n in names:
        np.testing.assert_array_equal(np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n))
    assert bench.DUMP_BUDGET <= 64 << 20
