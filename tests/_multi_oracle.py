"""Training losses of a batch with k images per domain, composed from the pieces of oracle/model_ref.py.

model_ref.training_losses restates the reference's step for its own batches, [source, target] and [source, target,
auxiliary].  This module restates the project's extension to k images per domain, [S_1..S_k, T_1..T_k(, A_1..A_k)], with
the SAME pieces — backbone_c4, rpn_head, rpn_proposals, rpn_losses, box_head_pass, img_head, ins_head, img_bce, adv_weight
and the gradient-reversal function — and nothing of its own but the k-wide slices and the consistency term taken per
image:
  * consistency: every instance row against the spatial mean of ITS image's sigmoid map (the docstring formula of
    layers/consistency_loss.py:3-12; rows are stacked in image order, the counts come from the DA sample);
  * image triplet: F.triplet_margin_loss(f[0:k], f[k:2k], f[2k:3k]) — distance over W, mean over (k, C, H);
  * triplet detection / DA passes on f[0:2k], proposals[0:2k], targets[0:2k];
  * ALIGNMENT: box_head_pass(f[d k:(d + 1) k], proposals[k:2k], targets[d k:(d + 1) k]) for d = 0, 1, 2.
At k = 1 every expression is model_ref's own, operand for operand: tests/test_multi_image_host.py requires the two to
agree to the last bit on the golden cases, and that is what makes this an oracle at k = 2."""
import torch
import torch.nn.functional as F

from oracle import model_ref as M


def images_per_domain(gts, domains):
    src = [bool(g["is_source"].any()) for g in gts]
    k = sum(src)
    assert k > 0 and all(src[:k]) and len(gts) == domains * k, src
    return k


def consistency_rows(img_sig, ins_sig, rows_per_image):
    """|mean_hw(img_sig[i]) - ins_sig[j]| for row j of image i, mean over the rows (one level)"""
    means = img_sig.reshape(img_sig.shape[0], -1).mean(1)
    assert len(rows_per_image) == means.shape[0] and sum(rows_per_image) == ins_sig.size(0)
    rows = torch.cat([means[i].view(1, 1).repeat(n, 1) for i, n in enumerate(rows_per_image)], 0)
    return torch.abs(rows - ins_sig).mean()


def da_losses_plain(feat, ins_feat, ins_labels, img_labels, rows_per_image, sd, cfg, draws=None):
    """model_ref.da_losses_plain with the per-image consistency rows"""
    da = cfg.MODEL.DA_HEADS
    p = "da_heads"
    v = F.avg_pool2d(ins_feat, 7).flatten(1)
    img_logits = M.img_head(M._GRL.apply(feat, -da.DA_IMG_GRL_WEIGHT), sd, p)
    ins_logits = M.ins_head(M._GRL.apply(v, -da.DA_INS_GRL_WEIGHT), sd, p, draws=draws)
    img_cst = M.img_head(M._GRL.apply(feat, da.DA_IMG_GRL_WEIGHT), sd, p).sigmoid()
    ins_cst = M.ins_head(M._GRL.apply(v, da.DA_INS_GRL_WEIGHT), sd, p, draws=draws).sigmoid()
    out = {}
    if da.DA_IMG_LOSS_WEIGHT > 0:
        out["loss_da_image"] = da.DA_IMG_LOSS_WEIGHT * M.img_bce(img_logits, img_labels)
    if da.DA_INS_LOSS_WEIGHT > 0:
        out["loss_da_instance"] = da.DA_INS_LOSS_WEIGHT * F.binary_cross_entropy_with_logits(
            ins_logits.squeeze(), ins_labels.float())
    if da.DA_CST_LOSS_WEIGHT > 0:
        out["loss_da_consistency"] = da.DA_CST_LOSS_WEIGHT * consistency_rows(img_cst, ins_cst, rows_per_image)
    return out


def da_losses_triplet(feat2, ins_feat, ins_labels, img_labels, rows_per_image, feat3, k, ins_set, state, sd, cfg,
                      draws=None):
    """model_ref.da_losses_triplet with the k-wide image triplet and the per-image consistency rows"""
    da = cfg.MODEL.DA_HEADS
    p = "da_heads_triplet"
    out = {}
    if da.DA_TRIPLET_INS_WEIGHT > 0:
        s, q, n = [F.avg_pool2d(f, 7).flatten(1) for f in ins_set]
        state["margin_ins"] = da.TRIPLET_MARGIN_INS
        loss = F.triplet_margin_loss(s, q, n, margin=state["margin_ins"], p=2)
        out["triplet_loss_instance"] = da.DA_TRIPLET_INS_WEIGHT * loss
    if da.DA_TRIPLET_IMG_WEIGHT > 0:
        if state.get("margin_img", 0.0) == 0.0:
            state["margin_img"] = da.TRIPLET_MARGIN_IMG
        if state.get("prev_img", 1) == 0.0 and int(state["margin_img"]) != int(da.TRIPLET_MAX_MARGIN):
            state["margin_img"] += 0.001
        loss = F.triplet_margin_loss(feat3[0:k], feat3[k:2 * k], feat3[2 * k:3 * k], margin=state["margin_img"], p=2)
        out["triplet_loss_image"] = da.DA_TRIPLET_IMG_WEIGHT * loss
        state["prev_img"] = float(loss.detach())
    if da.DA_IMG_LOSS_WEIGHT > 0:
        cur = M.img_bce(M.img_head(feat2, sd, p).detach(), img_labels)
        w = M.adv_weight(cur, da.DA_IMG_GRL_WEIGHT, da.DA_IMG_advGRL_WEIGHT, da.DA_ADV_GRL_THRESHOLD) \
            if da.DA_ADV_GRL else -da.DA_IMG_GRL_WEIGHT
        out["loss_da_image"] = da.DA_IMG_LOSS_WEIGHT * M.img_bce(M.img_head(M._GRL.apply(feat2, w), sd, p), img_labels)
    v = F.avg_pool2d(ins_feat, 7).flatten(1)
    if da.DA_INS_LOSS_WEIGHT > 0:
        cur = F.binary_cross_entropy_with_logits(M.ins_head(v.detach(), sd, p, draws=draws).squeeze(), ins_labels.float())
        w = M.adv_weight(cur, da.DA_INS_GRL_WEIGHT, da.DA_INS_advGRL_WEIGHT, da.DA_ADV_GRL_THRESHOLD) \
            if da.DA_ADV_GRL else -da.DA_INS_GRL_WEIGHT
        out["loss_da_instance"] = da.DA_INS_LOSS_WEIGHT * F.binary_cross_entropy_with_logits(
            M.ins_head(M._GRL.apply(v, w), sd, p, draws=draws).squeeze(), ins_labels.float())
    if da.DA_CST_LOSS_WEIGHT > 0:
        img_cst = M.img_head(M._GRL.apply(feat2, da.DA_IMG_GRL_WEIGHT), sd, p).sigmoid()
        ins_cst = M.ins_head(M._GRL.apply(v, da.DA_INS_GRL_WEIGHT), sd, p, draws=draws).sigmoid()
        out["loss_da_consistency"] = da.DA_CST_LOSS_WEIGHT * consistency_rows(img_cst, ins_cst, rows_per_image)
    return out


def training_losses(sd, cfg, images, gts, state=None, intermediates=None, selection_maps=None, draws=None,
                    selection_proposals=None):
    """model_ref.training_losses for [S_1..S_k, T_1..T_k(, A_1..A_k)]; same arguments, same order of random draws"""
    N, _, H, W = images.shape
    triplet = bool(cfg.MODEL.DA_HEADS.TRIPLET_USE)
    k = images_per_domain(gts, 3 if triplet else 2)
    image_sizes = [(H, W)] * N
    feat = M.backbone_c4(images, sd)
    objectness, deltas = M.rpn_head(feat, sd)
    rpn = cfg.MODEL.RPN
    anchors = M.grid_anchors(feat.shape[2], feat.shape[3], rpn.ANCHOR_STRIDE[0],
                             M.cell_anchors(rpn.ANCHOR_STRIDE[0], rpn.ANCHOR_SIZES, rpn.ASPECT_RATIOS))
    with torch.no_grad():
        sel_obj, sel_del = selection_maps if selection_maps is not None else (objectness, deltas)
        if sel_obj.shape[0] < N:
            lead = sel_obj.shape[0]
            sel_obj = torch.cat([sel_obj.to(objectness.dtype), objectness[lead:].detach()], dim=0)
            sel_del = torch.cat([sel_del.to(deltas.dtype), deltas[lead:].detach()], dim=0)
        proposals = M.rpn_proposals(sel_obj, sel_del, anchors, image_sizes, gts, cfg, True)
        if selection_proposals is not None:
            proposals = [p if q is None else (q[0].to(p[0].dtype), q[1].to(p[1].dtype))
                         for p, q in zip(proposals, list(selection_proposals) + [None] * (N - len(selection_proposals)))]
    obj_loss, rpn_box_loss = M.rpn_losses(objectness, deltas, anchors, image_sizes, gts, cfg, draws, intermediates)
    img_labels = torch.tensor([1.0 if g["is_source"].any() else 0.0 for g in gts])
    losses = {}
    if triplet:
        det, da_feat, dom, samples, da_samples = M.box_head_pass(feat[0:2 * k], proposals[0:2 * k], gts[0:2 * k], sd, cfg,
                                                                 draws=draws)
        ins_set = None
        if cfg.MODEL.DA_HEADS.ALIGNMENT:
            ins_set = []
            for d in range(3):
                _, f_d, _, _, _ = M.box_head_pass(feat[d * k:(d + 1) * k], proposals[k:2 * k], gts[d * k:(d + 1) * k], sd,
                                                  cfg, draws=draws)
                ins_set.append(f_d)
        rows = [len(s["boxes"]) for s in da_samples]
        da = da_losses_triplet(feat[0:2 * k], da_feat, dom, img_labels[0:2 * k], rows, feat, k, ins_set,
                               state if state is not None else {}, sd, cfg, draws)
    else:
        det, da_feat, dom, samples, da_samples = M.box_head_pass(feat, proposals, gts, sd, cfg, draws=draws)
        rows = [len(s["boxes"]) for s in da_samples]
        da = da_losses_plain(feat, da_feat, dom, img_labels, rows, sd, cfg, draws)
    losses.update(det)
    losses.update({"loss_objectness": obj_loss, "loss_rpn_box_reg": rpn_box_loss})
    losses.update(da)
    if intermediates is not None:
        intermediates.update(feat=feat.detach(), objectness=objectness.detach(), deltas=deltas.detach(),
                             proposals=[(b.clone(), s.clone()) for b, s in proposals],
                             sampled_idx=[s["idx"] for s in samples], da_sampled_idx=[s["idx"] for s in da_samples],
                             da_feat=da_feat.detach(), rows_per_image=rows)
    return losses


def first_seed_with_distinct_scores(case, k, H, W):
    """the first seed >= 0 (seeded weights of golden/fill.py, synthetic batch of that seed) at which the sigmoid objectness
    values of this restatement are pairwise distinct within each image, as tests/golden/make_golden.py chooses its seeds:
    the order of tied scores is unspecified.  `PYTHONPATH=.:tests python tests/_multi_oracle.py` prints the seeds that
    tests/test_multi_image_model_gpu.py uses."""
    from da_detect_amd.data.synthetic import make_batch
    from da_detect_amd.modeling.detector import build_detection_model
    from golden.cases import case_cfg
    from golden.fill import fill_state_dict

    c = case_cfg(case)
    n_img = (3 if c.MODEL.DA_HEADS.TRIPLET_USE else 2) * k
    blank = build_detection_model(c).state_dict()
    seed = 0
    while True:
        sd = fill_state_dict(blank, seed)
        images, _ = make_batch(c, n_img, H, W, seed=seed, device=torch.device("cpu"), num_source=k)
        with torch.no_grad():
            objectness, _ = M.rpn_head(M.backbone_c4(images.tensors, sd), sd)
        flat = objectness.permute(0, 2, 3, 1).reshape(n_img, -1).sigmoid()
        if all(torch.unique(flat[i]).numel() == flat[i].numel() for i in range(n_img)):
            return seed
        seed += 1


if __name__ == "__main__":
    print("da_plain, k = 2, 192 x 320:", first_seed_with_distinct_scores("da_plain", 2, 192, 320))
    print("da_triplet_aligned, k = 2, 160 x 288:", first_seed_with_distinct_scores("da_triplet_aligned", 2, 160, 288))
