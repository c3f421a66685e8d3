"""Host side of training with k images per domain ([S_1..S_k, T_1..T_k(, A_1..A_k)]): the generalised consistency loss, the
synthetic batches, the batch check, the count of images whose proposals are read, and the pin of tests/_multi_oracle.py to
oracle/model_ref.py at k = 1.  No GPU."""
import os
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


# ----------------------------------------------------------------------------------------------- consistency loss
def _cst_inputs(rows_per_image, levels, seed):
    g = torch.Generator().manual_seed(seed)
    n_img, R = len(rows_per_image), sum(rows_per_image)
    maps = [torch.rand((n_img, 1, 3 + l, 5), generator=g) for l in range(levels)]     # per-level probability maps
    ins = torch.rand((R, 1), generator=g)
    return maps, ins


@pytest.mark.parametrize("levels", [1, 3])
@pytest.mark.parametrize("rows_per_image", [(3, 4), (2, 0, 4, 1), (1, 1, 1, 1, 1, 1)], ids=str)
def test_consistency_loss_per_image_against_float64(rows_per_image, levels):
    """|mean_hw p_img[l][i] - p_ins[j]| for row j of image i, mean over rows x levels, written out in float64.  fp32: a mean
    of HW <= 25 values, one subtraction, a mean of R * L <= 21 terms in [0, 1]: well inside 64 u."""
    from da_detect_amd.layers.misc import consistency_loss

    maps, ins = _cst_inputs(rows_per_image, levels, 5)
    labels = torch.zeros(ins.shape[0])
    for img_feas in (maps, [m.reshape(m.shape[0], -1).mean(1) for m in maps]):      # maps, or (fused path) their means
        got = consistency_loss(img_feas, ins, labels, size_average=True, rows_per_image=rows_per_image)
        total, j = 0.0, 0
        for i, n in enumerate(rows_per_image):
            for _ in range(n):
                for m in maps:
                    total += abs(float(m[i].double().mean()) - float(ins[j, 0].double()))
                j += 1
        want = total / (sum(rows_per_image) * levels)
        assert abs(float(got) - want) <= 64 * 2.0 ** -24, (float(got), want)
        got_sum = consistency_loss(img_feas, ins, labels, size_average=False, rows_per_image=rows_per_image)
        assert abs(float(got_sum) - total) <= 64 * 2.0 ** -24 * max(total, 1.0)


def test_consistency_loss_two_images_is_the_old_call():
    from da_detect_amd.layers.misc import consistency_loss

    maps, ins = _cst_inputs((3, 4), 3, 9)
    labels = torch.tensor([1.0, 1, 1, 0, 0, 0, 0])
    old = consistency_loss(maps, ins, labels)
    labels._n_src_host = 3                        # what the box head attaches
    assert torch.equal(consistency_loss(maps, ins, labels), old)
    assert torch.equal(consistency_loss(maps, ins, labels, rows_per_image=(3, 4)), old)


def test_consistency_loss_three_images_without_rows_keeps_the_old_refusal():
    from da_detect_amd.layers.misc import consistency_loss

    maps, ins = _cst_inputs((2, 2, 3), 1, 1)
    with pytest.raises(AssertionError, match="only batch size=2 is supported for consistency loss now, received batch "
                                             "size: 3"):
        consistency_loss(maps, ins, torch.tensor([1.0, 1, 0, 0, 0, 0, 0]))
    with pytest.raises(ValueError):
        consistency_loss(maps, ins, torch.zeros(7), rows_per_image=(2, 2, 2))        # 6 rows described, 7 given
    with pytest.raises(ValueError):
        consistency_loss(maps, ins, torch.zeros(7), rows_per_image=(3, 4))           # two images described, three given


# ------------------------------------------------------------------------------------------------ synthetic batches
def test_make_batch_num_source():
    from da_detect_amd.config import cfg
    from da_detect_amd.data.synthetic import make_batch, make_targets
    from da_detect_amd.structures.bounding_box import is_source_image

    cpu = torch.device("cpu")
    for n in (2, 3, 4):
        a_img, a_tg = make_batch(cfg, n, 64, 96, seed=3, device=cpu)
        b_img, b_tg = make_batch(cfg, n, 64, 96, seed=3, device=cpu, num_source=1)
        assert torch.equal(a_img.tensors, b_img.tensors) and a_img.image_sizes == b_img.image_sizes
        for s, t in zip(a_tg, b_tg):
            assert torch.equal(s.bbox, t.bbox) and s.size == t.size and s.mode == t.mode
            assert sorted(s.fields()) == sorted(t.fields())
            for f in s.fields():
                assert torch.equal(s.get_field(f), t.get_field(f))
        assert [bool(is_source_image(t)) for t in a_tg] == [True] + [False] * (n - 1)
    _, tg = make_batch(cfg, 6, 64, 96, seed=3, device=cpu, num_source=2)
    assert [bool(is_source_image(t)) for t in tg] == [True, True, False, False, False, False]
    one = make_targets(4, 64, 96, 9, 3)
    two = make_targets(4, 64, 96, 9, 3, num_source=2)
    for s, t in zip(one, two):          # only the flags differ
        assert torch.equal(s.bbox, t.bbox) and torch.equal(s.get_field("labels"), t.get_field("labels"))


# ------------------------------------------------------------------------------------------------------ batch check
def _targets(layout):
    from da_detect_amd.data.synthetic import make_targets

    tg = make_targets(len(layout), 64, 96, 9, 1)
    for t, d in zip(tg, layout):
        t.add_field("is_source", torch.full((len(t),), d == "S", dtype=torch.bool))
    return tg


@pytest.mark.parametrize("layout,domains,k", [("ST", 2, 1), ("SSTT", 2, 2), ("SSSSTTTT", 2, 4), ("STA", 3, 1),
                                              ("SSTTAA", 3, 2)])
def test_batch_check_accepts_k_images_per_domain(layout, domains, k):
    from da_detect_amd.modeling.elision import images_per_domain

    assert images_per_domain(_targets(layout), domains) == k


@pytest.mark.parametrize("layout,domains", [("STT", 2), ("STST", 2), ("SSTTA", 3), ("TS", 2), ("TT", 2), ("SST", 3)])
def test_batch_check_refuses(layout, domains):
    from da_detect_amd.modeling.elision import images_per_domain

    with pytest.raises(ValueError, match="DA batch"):
        images_per_domain(_targets(layout), domains)


def test_model_raises_value_error_on_a_bad_batch():
    """GeneralizedRCNN.forward checks the batch before the backbone runs (a stub stands in for it: reaching it is the
    failure)"""
    from da_detect_amd.modeling.detector.generalized_rcnn import GeneralizedRCNN

    def boom(*a, **k):
        raise RuntimeError("the backbone ran")

    for layout, triplet in (("STT", False), ("STST", False), ("SSTTA", True)):
        m = types.SimpleNamespace(training=True, da_heads=not triplet, da_heads_triplet=triplet, backbone=boom,
                                  rpn=types.SimpleNamespace())
        images = torch.zeros((len(layout), 3, 64, 96))
        with pytest.raises(ValueError, match="DA batch"):
            GeneralizedRCNN.forward(m, images, _targets(layout))


# -------------------------------------------------------------------------------------- images with read proposals
@pytest.mark.parametrize("k", [1, 2])
def test_images_with_read_proposals(k):
    from da_detect_amd.modeling.detector.generalized_rcnn import GeneralizedRCNN

    f = GeneralizedRCNN._images_with_read_proposals
    plain, trip = _targets("S" * k + "T" * k), _targets("S" * k + "T" * k + "A" * k)
    heads = lambda need: types.SimpleNamespace(needs_instance_features=need)        # noqa: E731
    m = lambda **kw: types.SimpleNamespace(**kw)                                    # noqa: E731
    assert f(m(da_heads_triplet=False, da_heads=heads(True), Aligned=False), plain) == 2 * k
    assert f(m(da_heads_triplet=False, da_heads=heads(False), Aligned=False), plain) == k
    assert f(m(da_heads_triplet=heads(True), da_heads=heads(True), Aligned=False), trip) == 2 * k
    assert f(m(da_heads_triplet=heads(False), da_heads=heads(True), Aligned=True), trip) == 2 * k
    assert f(m(da_heads_triplet=heads(False), da_heads=heads(True), Aligned=False), trip) == k
    # a triplet module fed a batch that is no [S.., T.., A..]: nothing is assumed
    assert f(m(da_heads_triplet=heads(True), da_heads=heads(True), Aligned=False), plain + plain[:1]) is None
    assert f(m(da_heads_triplet=False, da_heads=heads(True), Aligned=False), _targets("T" * k + "S" * k)) is None


# ------------------------------------------------------------------------------------ the oracle helper, pinned at k = 1
@pytest.mark.parametrize("case", ["da_plain", "da_triplet_aligned"])
def test_multi_oracle_is_model_ref_at_k1(case):
    """tests/_multi_oracle.py composes the pieces of oracle/model_ref.py with k-wide slices; at k = 1 (the golden cases, on
    their fixtures' RPN maps) every loss equals model_ref.training_losses' to the last bit, and so do the sampled rows"""
    import _multi_oracle
    from da_detect_amd.data.synthetic import make_batch
    from da_detect_amd.modeling.detector import build_detection_model
    from golden.cases import case_cfg
    from golden.fill import fill_state_dict
    from oracle import model_ref

    z = np.load(os.path.join(GOLD, case + ".npz"))
    c = case_cfg(case)
    seed, H, W, nimg = int(z["seed"]), int(z["H"]), int(z["W"]), int(z["nimg"])
    sd = fill_state_dict(build_detection_model(c).state_dict(), seed)
    images, targets = make_batch(c, nimg, H, W, seed=seed, device=torch.device("cpu"))
    gts = model_ref.targets_to_dicts(targets)
    maps = (torch.from_numpy(z["objectness"]), torch.from_numpy(z["deltas"]))
    out = []
    for fn in (model_ref.training_losses, _multi_oracle.training_losses):
        inter = {}
        torch.manual_seed(seed)
        with torch.no_grad():
            losses = fn(sd, c, images.tensors, gts, state={}, intermediates=inter, selection_maps=maps)
        out.append((losses, inter))
    (a, ia), (b, ib) = out
    assert set(a) == set(b) and len(a) >= 6
    for k in a:
        assert torch.equal(a[k], b[k]), (k, float(a[k]), float(b[k]))
    for x, y in zip(ia["da_sampled_idx"], ib["da_sampled_idx"]):
        assert torch.equal(x, y)
    assert ib["rows_per_image"] == [len(i) for i in ia["da_sampled_idx"]]
