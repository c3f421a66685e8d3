"""MODEL.BACKBONE.FREEZE_CONV_BODY_AT: which parameters of the R-50-C4 model train at each level (no kernels are launched).

The reference's rule (maskrcnn_benchmark/modeling/backbone/resnet.py:127-136): the stages 0 .. freeze_at - 1 of the backbone
body are frozen, stage 0 being the stem and stage i being layer{i}; nothing outside the body is touched, and a level of 0
or below freezes nothing."""
import re

import pytest


def _stage_of(name):
    """backbone stage a parameter belongs to, None outside the backbone body (heads, RPN, the res5 ROI head)"""
    m = re.match(r"backbone\.body\.(stem|layer(\d+))\.", name)
    if m is None:
        return None
    return 0 if m.group(1) == "stem" else int(m.group(2))


@pytest.mark.parametrize("freeze_at", [-1, 0, 1, 2, 3])
def test_trainable_parameters_follow_the_reference_rule(freeze_at):
    from da_detect_amd.modeling.detector import build_detection_model
    from golden.cases import case_cfg

    c = case_cfg("da_plain")
    assert c.MODEL.BACKBONE.CONV_BODY == "R-50-C4"
    c.merge_from_list(["MODEL.BACKBONE.FREEZE_CONV_BODY_AT", freeze_at])
    model = build_detection_model(c)         # raises nothing at any level
    names = [n for n, _ in model.named_parameters()]
    assert {_stage_of(n) for n in names} == {None, 0, 1, 2, 3}
    want = {n for n in names if _stage_of(n) is None or _stage_of(n) >= freeze_at}
    got = {n for n, p in model.named_parameters() if p.requires_grad}
    assert got == want, sorted(got ^ want)
    # res2 consumes the max-pooled map, whose ReLU gate belongs to the stem's backward, at every level
    assert model.backbone.body.layer1.input_is_relu is False
    assert all(getattr(model.backbone.body, "layer%d" % i).input_is_relu for i in (2, 3))
