"""R-50-C4 training steps with k = 2 images per domain on the default (benchmarked) GPU path, under the CPU oracle.

The scheme is tests/test_default_path_gpu.py's: seeded weights (golden/fill.py), the synthetic batch of the seed, one
train_step with the device samplers; the test records the 64-bit seeds handed to the sampler kernels, the dropout masks,
the RPN maps and the proposal lists, and the oracle replays them.  The harness is that file's `_run_default_path`, with its
batch maker widened to [S_1, S_2, T_1, T_2(, A_1, A_2)]; the oracle is tests/_multi_oracle.py — oracle/model_ref.py's pieces
with k-wide slices and per-image consistency rows, pinned to model_ref bit for bit at k = 1 (tests/test_multi_image_host.py)
— in float32, as test_default_path_matches_oracle_512x1024 runs model_ref for the same bar on the losses (its own rounding
is two orders below the bar).

Seeds: the first seed >= 0 at which the oracle's sigmoid objectness values are pairwise distinct within each image, as
tests/golden/make_golden.py takes them (_multi_oracle.first_seed_with_distinct_scores, found on the CPU): 8 for the plain
batch of four 192 x 320 images, 0 for the triplet batch of six 160 x 288 images.

Bar: every loss within the project's 1e-4 (relative, floor 1) of the oracle: abs(got - ref) <= 1e-4 * max(abs(ref), 1).
64 sampled ROIs per image (the sampler rule and the kernels do not depend on the cap; test_default_path_gpu.py does the same
for the aligned recipe): a quarter of the oracle's res5 passes."""
import pytest
import torch

from test_default_path_gpu import _check_losses, _run_default_path

pytestmark = pytest.mark.gpu
K = 2
ROIS = ("MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 64)
PLAIN = ("da_plain", 192, 320, 8, ROIS)
TRIPLET = ("da_triplet_aligned", 160, 288, 0, ROIS)          # ALIGNMENT, DA_TRIPLET_INS_WEIGHT 1.0, DA_CST_LOSS_WEIGHT 0.1


def _make_batch_k(monkeypatch):
    """the harness asks for 2 (3) images; hand it K per domain, the first K marked as source"""
    from da_detect_amd.data import synthetic

    orig = synthetic.make_batch

    def make_batch(cfg, num_images, height, width, seed, device):
        assert num_images in (2, 3)
        return orig(cfg, num_images * K, height, width, seed=seed, device=device, num_source=K)

    monkeypatch.setattr(synthetic, "make_batch", make_batch)
    return orig


def _run(spec, device, monkeypatch):
    case, H, W, seed, overrides = spec
    orig = _make_batch_k(monkeypatch)
    c, sd, rec, domains = _run_default_path(case, H, W, device, seed, monkeypatch, overrides)
    monkeypatch.setattr("da_detect_amd.data.synthetic.make_batch", orig)
    return c, sd, rec, domains * K


def _oracle_losses(c, sd, rec, nimg, H, W, seed):
    import _multi_oracle
    from da_detect_amd.data.synthetic import make_batch
    from oracle import model_ref

    osd = {k: v.clone() for k, v in sd.items()}
    cpu_images, cpu_targets = make_batch(c, nimg, H, W, seed=seed, device=torch.device("cpu"), num_source=K)
    draws = model_ref.DeviceDraws(rec["seeds"], rec["masks"])
    inter = {}
    with torch.no_grad():
        losses = _multi_oracle.training_losses(osd, c, cpu_images.tensors, model_ref.targets_to_dicts(cpu_targets),
                                               state={}, intermediates=inter, draws=draws,
                                               selection_maps=(rec["objectness"].cpu(), rec["deltas"].cpu()),
                                               selection_proposals=rec["proposals"])
    assert draws.exhausted(), "the oracle consumed %d/%d seeds and %d/%d dropout masks" % (
        draws.taken_seeds, len(draws.seeds), draws.taken_masks, len(draws.masks))
    return losses, inter


def _print(rec, olosses):
    for k, v in sorted(olosses.items()):
        v = float(v)
        print("    %-24s gpu %.7f  oracle %.7f  err / bar %.3f" % (k, rec["losses"][k], v,
                                                                   abs(rec["losses"][k] - v) / (1e-4 * max(abs(v), 1.0))))


def test_plain_da_two_images_per_domain(device, monkeypatch):
    """[S, S, T, T] of 192 x 320, image + instance + consistency losses: every loss against the oracle; the instance tail ran
    with four row segments"""
    from da_detect_amd import _C

    calls = []
    orig = _C.da_ins_tail_forward_n
    monkeypatch.setattr(_C, "da_ins_tail_forward_n", lambda *a: calls.append(a[-1]) or orig(*a))
    case, H, W, seed, _ = PLAIN
    c, sd, rec, nimg = _run(PLAIN, device, monkeypatch)
    assert c.MODEL.DA_HEADS.DA_INS_LOSS_WEIGHT > 0 and c.MODEL.DA_HEADS.DA_CST_LOSS_WEIGHT > 0
    assert nimg == 4 and rec["objectness"].shape[0] == 4 and len(rec["proposals"]) == 4
    assert len(calls) == 1 and len(calls[0]) == 4, calls
    olosses, inter = _oracle_losses(c, sd, rec, nimg, H, W, seed)
    assert list(calls[0]) == [sum(inter["rows_per_image"][:i + 1]) for i in range(4)]
    _print(rec, olosses)
    assert {"loss_da_image", "loss_da_instance", "loss_da_consistency"} <= set(olosses)
    _check_losses(rec, olosses)


def test_triplet_aligned_two_images_per_domain(device, monkeypatch):
    """[S, S, T, T, A, A] of 160 x 288 with ALIGNMENT: the auxiliary images get no RPN head pass, the box head sees four
    images, the three aligned passes two each; every loss against the oracle"""
    case, H, W, seed, _ = TRIPLET
    c, sd, rec, nimg = _run(TRIPLET, device, monkeypatch)
    da = c.MODEL.DA_HEADS
    assert da.ALIGNMENT and da.DA_TRIPLET_INS_WEIGHT == 1.0 and da.DA_CST_LOSS_WEIGHT == 0.1
    assert nimg == 6 and rec["objectness"].shape[0] == 4 and len(rec["proposals"]) == 4
    assert len(rec["rois"]) == 4 + 3 * 2, len(rec["rois"])
    olosses, _ = _oracle_losses(c, sd, rec, nimg, H, W, seed)
    _print(rec, olosses)
    assert {"triplet_loss_image", "triplet_loss_instance", "loss_da_consistency", "loss_da_instance"} <= set(olosses)
    _check_losses(rec, olosses)


def test_triplet_training_step_is_finite_and_repeatable(device, monkeypatch):
    """the same triplet batch through train_step twice from one seed: contraction mode 4's guard is clean after the backward,
    every trainable parameter has a finite gradient, and both runs give the same losses"""
    from da_detect_amd import _C

    runs = []
    for _ in range(2):
        _, _, rec, _ = _run(TRIPLET, device, monkeypatch)
        _C.check_nonfinite()
        assert rec["grads"] and all(bool(torch.isfinite(g).all()) for g in rec["grads"].values())
        assert all(v == v and abs(v) != float("inf") for v in rec["losses"].values())
        runs.append(dict(rec, seeds=list(rec["seeds"])))       # (the second run's hooks wrap the first's)
    assert runs[0]["seeds"] == runs[1]["seeds"]
    assert runs[0]["losses"] == runs[1]["losses"], (runs[0]["losses"], runs[1]["losses"])
