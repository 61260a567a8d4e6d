#!/usr/bin/env python3
"""Body-model path (SURVEY.md section 8 row f1 / config C4 per GPU: B=128 images x K=128 hypotheses of a 144-D 6D pose): time of the
Glow sampling pass, the 6D -> R conversion and the SMPL-sized linear-blend skinning (24 joints, 6,890 vertices), whole and for a
1/8 hypothesis slice (what one rank of a hypothesis-sharded 8-GPU job decodes).  Synthetic tables; parity unpinned at this size.
TRAIN=1 adds the train leg: forward + backward of the head in f32 (log_prob[:, 1:].mean() + a joint loss, joints only) next to the f32
forward-only time of the same call under no_grad.  VERTS=1 (with TRAIN=1) adds the vertex-loss leg: log_prob[:, 1:].mean() + |vertices - target|.mean()
with verts_grad=True, and the time of the skinning reverse alone (body.lbs_bwd) next to the forward skinning.
NLL=1 runs the maximum-likelihood leg INSTEAD of the sampling legs (B rows, one annotated pose per image; K is not used): forward-only
head.log_prob under no_grad, and forward + backward of -log_prob.mean(), both in f32, each as the median of WINDOWS (7) timing windows.  STEPS=n
(with NLL=1) runs n untimed forward + backward steps only (for a kernel trace).
Keypoints (NK = 17 rows of a synthetic regressor; always printed): route (a) want_verts=True + torch.einsum with the regressor, route (b)
want_verts=False, want_keypoints=True (accumulated inside the skinning pass), and the plain vertex call, as medians of WINDOWS alternating windows;
TRAIN=1 adds the train step of log_prob.mean() - keypoint_log_prob(...).mean() next to the step of log_prob.mean() alone.  KPONLY=1 stops after
the keypoint lines (for a kernel trace of the three routes).
EVAL=1 runs the evaluation leg INSTEAD of the other legs: head.evaluate(...) with target_verts (min-of-n MPJPE / PA-MPJPE / per-vertex error, no
vertex tensor) against the composition from the calls that existed before it - head(..., want_verts=True, want_keypoints=True), the same errors
in torch on the (B, K, NV, 3) tensor, ops.procrustes_align for the aligned error, torch.cummin for the minima - on the same noise, as medians of
WINDOWS alternating windows; prints the largest difference between the two routes' errors."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from mhentropy_amd import body, synth

B, K = int(os.environ.get("B", 128)), int(os.environ.get("K", 128))
NK = 17
head = body.BodyFlowHead(body.synthetic_body_tables(0, keypoints=NK), context_features=2048, hidden=1024, num_layers=4, num_blocks=2)
head.flow.load_state_dict({k: torch.as_tensor(v) for k, v in synth.glow_state(1, 144, 1024, 4, 2, 2048).items()}, strict=False)
head = head.cuda().eval()
head.flow.compute_dtype = torch.bfloat16 if os.environ.get("DT", "bf16") == "bf16" else torch.float32
feats = torch.randn(B, 2048, device="cuda") * 0.5
betas = torch.randn(B, 10, device="cuda")
noise = torch.randn(B, K, 144, device="cuda")


def t(fn, n=5):
    fn(); torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


if os.environ.get("NLL", "0") == "1":
    head.flow.compute_dtype = torch.float32
    pose6d = torch.randn(B, 144, device="cuda") * 0.8

    def nll_step():
        for p_ in head.flow.parameters():
            p_.grad = None
        (-head.log_prob(feats, pose6d=pose6d)[0].mean()).backward()

    def fwd():
        with torch.no_grad():
            head.log_prob(feats, pose6d=pose6d)

    head.train()                                   # (dropout p = 0: train mode only switches the differentiable pass on)
    if os.environ.get("STEPS"):
        for _ in range(int(os.environ["STEPS"])):
            nll_step()
        torch.cuda.synchronize()
        sys.exit(0)
    W = int(os.environ.get("WINDOWS", 7))
    fw = sorted(t(fwd, n=20) for _ in range(W))
    tr = sorted(t(nll_step, n=10) for _ in range(W))
    print(f"NLL leg (f32, one pose per image) B={B}: forward log_prob {fw[W // 2]:.3f} ms (min {fw[0]:.3f}, max {fw[-1]:.3f} over {W} windows) | "
          f"forward + backward {tr[W // 2]:.3f} ms (min {tr[0]:.3f}, max {tr[-1]:.3f}) = {tr[W // 2] / fw[W // 2]:.2f}x the forward")
    sys.exit(0)


if os.environ.get("EVAL", "0") == "1":
    from mhentropy_amd import ops
    ns, root, NV = (1, 5, 10, 25), (11, 12), head.body.NV
    tk, tv = torch.randn(B, NK, 3, device="cuda") * 0.3, torch.randn(B, NV, 3, device="cuda") * 0.3
    z = noise.clone()
    z[:, 0] = 0.0

    def fused():
        return head.evaluate(feats, K, tk, target_verts=tv, betas=betas, noise=noise, ns=ns, root=root)

    def composed():
        with torch.no_grad():
            out = head(feats, K, betas=betas, noise=z, want_verts=True, want_keypoints=True)
            kp, r = out["keypoints"], list(root)
            cen, tcen = kp[:, :, r].mean(2, keepdim=True), tk[:, r].mean(1, keepdim=True)
            res = {"mpjpe": ((kp - cen) - (tk - tcen)[:, None]).norm(dim=-1).mean(-1)}
            al = ops.procrustes_align(kp.permute(1, 0, 2, 3).contiguous(), tk).permute(1, 0, 2, 3)
            res["pa_mpjpe"] = (al - tk[:, None]).norm(dim=-1).mean(-1)
            res["pve"] = ((out["vertices"] - cen) - (tv - tcen)[:, None]).norm(dim=-1).mean(-1)
            for k in ("mpjpe", "pa_mpjpe", "pve"):
                cm = torch.cummin(res[k], 1)
                res["min_" + k], res["argmin_" + k] = cm.values[:, [n - 1 for n in ns]], cm.indices[:, [n - 1 for n in ns]]
        return res

    a_, b_ = fused(), composed()
    diff = {k: float((a_[k] - b_[k]).abs().max()) for k in ("mpjpe", "pa_mpjpe", "pve", "min_pve")}
    del a_, b_
    W = int(os.environ.get("WINDOWS", 7))
    tf, tc = [], []
    for _ in range(W):
        tf.append(t(fused, n=5)); tc.append(t(composed, n=5))
    tf, tc = sorted(tf), sorted(tc)
    print(f"EVAL leg B={B} K={K} NK={NK} NV={NV} ns={ns} (flow {os.environ.get('DT', 'bf16')}; median of {W} alternating windows of 5 [min, max]): "
          f"head.evaluate (fused mesh error, no vertex tensor) {tf[W // 2]:.3f} ms [{tf[0]:.3f}, {tf[-1]:.3f}] | composition (vertices + torch errors) "
          f"{tc[W // 2]:.3f} ms [{tc[0]:.3f}, {tc[-1]:.3f}] = {tc[W // 2] / tf[W // 2]:.2f}x the fused call | max |fused - composed|: "
          + ", ".join(f"{k} {v:.2e}" for k, v in diff.items()))
    sys.exit(0)


with torch.no_grad():
    pose, logp, _ = head.flow.sample_and_log_prob(K, noise=noise, context=feats)
    p = pose.reshape(B * K, 144).contiguous()
    bt = betas[:, None, :].expand(B, K, 10).reshape(B * K, 10).contiguous()
    R = B * K
    ms_flow = t(lambda: head.flow.sample_and_log_prob(K, noise=noise, context=feats))
    ms_rot = t(lambda: body.rot6d_to_rotmat(p.view(R, 24, 6)))
    rm = body.rot6d_to_rotmat(p.view(R, 24, 6))
    ms_lbs = t(lambda: head.body(bt, rotmats=rm))
    ms_joints = t(lambda: head.body(bt, rotmats=rm, want_verts=False))
    ms_all = t(lambda: head(feats, K, betas=betas, noise=noise))
    ms_slice = t(lambda: head(feats, K, betas=betas, noise=noise, hyp_slice=(0, K // 8)))
    # keypoints: what a caller could do before (vertices + a product the caller writes) against the fused pass; alternating windows, medians
    reg = head.body.keypoint_regressor
    route_a = lambda: torch.einsum("kv,rvc->rkc", reg, head.body(bt, rotmats=rm)["vertices"])
    route_b = lambda: head.body(bt, rotmats=rm, want_verts=False, want_keypoints=True)["keypoints"]
    route_v = lambda: head.body(bt, rotmats=rm)["vertices"]
    route_vk = lambda: head.body(bt, rotmats=rm, want_keypoints=True)["keypoints"]
    dkp = float((route_a() - route_b()).abs().max())
    W = int(os.environ.get("WINDOWS", 7))
    tw = {k: [] for k in "abvk"}
    for _ in range(W):
        for k, fn in (("a", route_a), ("b", route_b), ("v", route_v), ("k", route_vk)):
            tw[k].append(t(fn, n=10))
    md = {k: sorted(v)[W // 2] for k, v in tw.items()}
    rng_ = {k: (min(v), max(v)) for k, v in tw.items()}
vb = R * 6890 * 12
print(f"keypoints NK={NK} R={R} (median of {W} windows [min, max]): (a) vertices + einsum {md['a']:.3f} ms [{rng_['a'][0]:.3f}, {rng_['a'][1]:.3f}] | "
      f"(b) fused, no vertex tensor {md['b']:.3f} ms [{rng_['b'][0]:.3f}, {rng_['b'][1]:.3f}] = {md['b'] / md['a']:.3f}x of (a) | max |a - b| {dkp:.2e}")
print(f"keypoints NK={NK} R={R}: vertices alone {md['v']:.3f} ms [{rng_['v'][0]:.3f}, {rng_['v'][1]:.3f}] | vertices + fused keypoints "
      f"{md['k']:.3f} ms [{rng_['k'][0]:.3f}, {rng_['k'][1]:.3f}]")
if os.environ.get("KPONLY", "0") == "1":
    sys.exit(0)
print(f"B={B} K={K} R={R}: glow sample+log_prob {ms_flow:.2f} ms | rot6d {ms_rot * 1e3:.0f} us | LBS 6,890 verts {ms_lbs:.2f} ms "
      f"({vb / ms_lbs / 1e6:.0f} GB/s of vertices written, {R * 6890 * 3 * (10 + 207 + 96 + 4) / ms_lbs / 1e9:.1f} TFMA/s) | joints only {ms_joints * 1e3:.0f} us")
print(f"whole head {ms_all:.2f} ms = {R / ms_all * 1e3:.3e} hypotheses/s ; decoding a 1/8 hypothesis slice {ms_slice:.2f} ms")


if os.environ.get("TRAIN", "0") == "1":
    head.flow.compute_dtype = torch.float32
    head.train()                                   # (dropout p = 0: train mode only switches the differentiable pass on)
    target = torch.randn(B, K, 24, 3, device="cuda") * 0.3

    def step():
        for p_ in head.flow.parameters():
            p_.grad = None
        out = head(feats, K, betas=betas, noise=noise, want_verts=False)
        (out["log_prob"][:, 1:].mean() + (out["joints"] - target).abs().mean()).backward()

    with torch.no_grad():
        ms_fwd32 = t(lambda: head(feats, K, betas=betas, noise=noise, want_verts=False))
    ms_train = t(step, n=3)
    print(f"train leg (f32, joints only) B={B} K={K}: forward {ms_fwd32:.2f} ms | forward + backward {ms_train:.2f} ms "
          f"({ms_train / ms_fwd32:.2f}x the forward)")

    cam = torch.cat([torch.rand(B, 1, device="cuda") + 0.5, torch.randn(B, 2, device="cuda") * 0.1], 1)
    uv, vis = torch.randn(B, NK, 2, device="cuda") * 0.3, (torch.rand(B, NK, device="cuda") < 0.7).float()

    def kstep(with_kp):
        for p_ in head.flow.parameters():
            p_.grad = None
        out = head(feats, K, betas=betas, noise=noise, want_verts=False, want_keypoints=with_kp)
        loss = out["log_prob"].mean()
        if with_kp:
            loss = loss - body.keypoint_log_prob(out["keypoints"], cam, uv, vis).mean()
        loss.backward()

    ms_ent, ms_kp = t(lambda: kstep(False), n=3), t(lambda: kstep(True), n=3)
    print(f"train leg (f32, 2D keypoints) B={B} K={K} NK={NK}: log_prob.mean() alone {ms_ent:.2f} ms | log_prob.mean() - keypoint_log_prob.mean() "
          f"{ms_kp:.2f} ms (+{ms_kp - ms_ent:.2f} ms: fused keypoints, likelihood, keypoint + skinning reverse in {body.KP_BWD_ROWS}-row passes)")

    if os.environ.get("VERTS", "0") == "1":
        tv = torch.randn(B, K, 6890, 3, device="cuda") * 0.3

        def vstep():
            for p_ in head.flow.parameters():
                p_.grad = None
            out = head(feats, K, betas=betas, noise=noise, verts_grad=True)
            (out["log_prob"][:, 1:].mean() + (out["vertices"] - tv).abs().mean()).backward()

        with torch.no_grad():
            ms_fwdv = t(lambda: head(feats, K, betas=betas, noise=noise))
        ms_vtrain = t(vstep, n=3)
        gv = torch.randn(R, 6890, 3, device="cuda")
        ms_bwd = t(lambda: body.lbs_bwd(head.body, rm, bt, gv))
        ms_skin = t(lambda: head.body(bt, rotmats=rm))
        print(f"train leg (f32, vertex loss) B={B} K={K}: forward {ms_fwdv:.2f} ms | forward + backward {ms_vtrain:.2f} ms "
              f"({ms_vtrain / ms_fwdv:.2f}x the forward; joints only {ms_train:.2f} ms) | skinning reverse (lbs_bwd: pose pass + "
              f"both reductions + chain) {ms_bwd:.2f} ms vs forward LBS {ms_skin:.2f} ms ({ms_bwd / ms_skin:.2f}x)")
