"""Training entry point with the shape of the reference's `hand/run.py` -> `CrossModalHand.train()` loop
(hand/CrossModalHand.py:205-225 epochs + MultiStepLR, :430-470 iteration: training_step_start, model_forward =
get_loss + the N-sample metrics pass, criterion, backward/clip/Adam, AverageMeter bookkeeping, :573-587 checkpoint),
on synthetic batches (no dataset ships with this repository; the HO3D pipeline is out of scope).

    python -m mhentropy_amd.run --backbone resnet50 --batch 256 --hyps 64 --dtype bf16 --epochs 1 --iters 20
    python -m torch.distributed.run --nproc-per-node 8 -m mhentropy_amd.run ...      # one process per GPU, RCCL
    python -m mhentropy_amd.run --mods uv,xyz ...        # 3D-supervised training (hand/CrossModalHand.py:354, mods = ['xyz', 'uv'])
    python -m mhentropy_amd.run --chamfer-w 10 ...       # with the hand-object Chamfer term (hand/network.py:821-826, w_chamfer = 10)
    python -m mhentropy_amd.run --sil-w 1 ...            # with the silhouette term (the mesh against the hand mask, MHEnt.get_loss(sil_w=...))
    python -m mhentropy_amd.run --sil-w 1 --sil-occluder ...   # ... with the object's mask as the term's occluder (get_loss(sil_occluder=True))
    python -m mhentropy_amd.run --test-samples 200 --quant-samples 10 --quant kmeans ...      # metrics of 10 k-means modes of 200 hypotheses
    python -m mhentropy_amd.run --test-samples 200 --mesh-metrics ...       # HO3D mesh protocol: vertex error, F@5 / F@15 mm, aligned, best of N
    python -m mhentropy_amd.run --test-samples 200 --pck-metrics ...        # AUC of the 3D PCK curve 0..50 mm, joints and mesh, aligned, best of N
    python -m mhentropy_amd.run --test-samples 200 --depth-metrics ...      # depth agreement with the depth crop: top hypothesis, best of N, MPJPE of the pick
"""
import argparse
import json
import sys
import time

import torch

from . import dist as mdist, harness, synth
from .criteria import MHEntLoss
from .train import TrainStep


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--backbone", default="resnet50", choices=["resnet18", "resnet50"])
    ap.add_argument("--batch", type=int, default=64, help="images per GPU (configs/ho3d.yaml: 64)")
    ap.add_argument("--hyps", type=int, default=10, help="hypotheses per image in the loss (the reference hard-codes 10)")
    ap.add_argument("--test-samples", type=int, default=0, help="per-iteration metrics pass, training.test_samples (reference: 200)")
    ap.add_argument("--quant-samples", type=int, default=0,
                    help="cut the --test-samples hypotheses of the metrics pass to this many before the metrics, sample(N=[test_samples, "
                         "quant_samples]): the metrics are then quantised best-of-M (0: keep them all)")
    ap.add_argument("--quant", default="log_q", choices=["log_q", "kmeans"],
                    help="how --quant-samples cuts: log_q keeps the most likely hypotheses (the reference's N_quant), kmeans clusters the "
                         "hypotheses' joints into that many modes and keeps one representative of each (MHEnt.sample(quant='kmeans'))")
    ap.add_argument("--hidden", type=int, default=512)
    ap.add_argument("--flow-steps", type=int, default=6)
    ap.add_argument("--dtype", default="bf16", choices=["f32", "bf16"])
    ap.add_argument("--lr", type=float, default=2e-4)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--iters", type=int, default=10, help="iterations per epoch")
    ap.add_argument("--image-size", type=int, default=256)
    ap.add_argument("--milestones", type=int, nargs="*", default=[150, 250])
    ap.add_argument("--save", default="", help="write a checkpoint in the reference's container format here (rank 0)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cfg", default="", help="a YAML file in the reference's schema (hand/configs/ho3d.yaml): network / training sections "
                                              "override the flags above (backbone, h_dims, num_steps, batch_size, lr, milestones, test_samples)")
    ap.add_argument("--load", default="", help="checkpoint in the reference's container format to start from (training.pth)")
    ap.add_argument("--scalars", default="", help="write the reference's TensorBoard scalars here as JSON lines (rank 0)")
    ap.add_argument("--graph", type=int, default=0,
                    help="1: replay the whole iteration (forward, reverse, all-reduce, clip, Adam) from HIP graphs (train.GraphedStep; batches are "
                         "copied into static tensors, the graphs are re-captured when MultiStepLR changes the rate)")
    ap.add_argument("--input-pipeline", action="store_true",
                    help="feed the step from DECODED synthetic HO3D samples through the GPU input pipeline (ho3d_dataloader.HO3DBatchPipeline: "
                         "crop, augmentation, visibility, compute_st; hand/dataloader/ho3d_dataloader.py:272-459) instead of ready-made batches; "
                         "image size is then 256")
    ap.add_argument("--aligned", action="store_true",
                    help="report Procrustes-aligned 3D metrics (MHEntLoss(aligned=True), the reference's criteria.py:62-87): joints aligned to "
                         "pose3d, meshes to the target's verts where the batch carries them (--input-pipeline)")
    ap.add_argument("--mods", default="uv",
                    help="likelihoods of the loss, comma-separated (hand/CrossModalHand.py:354): uv (weak supervision, the reference's default), "
                         "uv,xyz or xyz (3D supervision: adds the Laplace likelihood of the normalised joints against the batch's pose3d)")
    ap.add_argument("--chamfer-w", type=float, default=0.0,
                    help="weight of the hand-object Chamfer term in the loss (hand/network.py:821-826: the reference's w_chamfer is 10, behind a "
                         "switch it ships off; 0 = off).  Synthetic objects (synth.object_targets) by default, the pipeline's object_verts "
                         "with object_count = the decoded samples' obj_count under --input-pipeline")
    ap.add_argument("--sil-w", type=float, default=0.0,
                    help="weight of the silhouette term in the loss (MHEnt.get_loss(sil_w=...): the distance of every hypothesis' projected mesh "
                         "to the image's hand mask; 0 = off).  Synthetic masks around the target keypoints (synth.hand_masks) by default, the "
                         "pipeline's hand_mask under --input-pipeline")
    ap.add_argument("--sil-occluder", action="store_true",
                    help="the silhouette term takes the object's mask as its occluder (MHEnt.get_loss(sil_occluder=True): a vertex behind the "
                         "object costs nothing, the object attracts nothing).  A synthetic disc or box over part of the hand mask, cut out of "
                         "it (synth.object_masks), by default, the pipeline's object_mask under --input-pipeline; needs --sil-w > 0")
    ap.add_argument("--mesh-metrics", action="store_true",
                    help="evaluate the meshes of the --test-samples metrics pass by the HO3D mesh protocol (criteria.mesh_eval: vertex error in mm "
                         "and F-score at 5 and 15 mm, plain and Procrustes-aligned, mean and best of N) and report them as mesh_err, mesh_err_pa, "
                         "f5, f15, f5_pa, f15_pa and *_best (the scalars log: metric_it/<name>).  The target mesh is the mesh of a seeded "
                         "ground-truth pose (synth.mesh_pose) by default, the pipeline's verts under --input-pipeline; needs --test-samples > 0")
    ap.add_argument("--pck-metrics", action="store_true",
                    help="evaluate the joints and meshes of the --test-samples metrics pass by the area under the 3D PCK curve from 0 to 50 mm "
                         "(criteria.pck_auc, 100 thresholds, plain and Procrustes-aligned, mean and best of N) and report them as auc_j, "
                         "auc_j_pa, auc_v, auc_v_pa and *_best (the scalars log: metric_it/<name>); the run's pooled AUC of the top hypothesis "
                         "(harness.PckPool: integer hits added over all iterations) is printed at the end.  The target mesh as for "
                         "--mesh-metrics: a seeded ground-truth pose by default, the pipeline's verts under --input-pipeline; needs "
                         "--test-samples > 0")
    ap.add_argument("--depth-metrics", action="store_true",
                    help="score the meshes of the --test-samples metrics pass against the depth crop (criteria.depth_dist, offset fitted per "
                         "hypothesis) and report depth_dist (the top hypothesis, metres), depth_dist_best (best of N) and depth_mpjpe (the MPJPE "
                         "in mm of the hypothesis the depth selects, next to epe3d) (the scalars log: metric_it/<name>).  The depth crop is "
                         "rendered from the mesh of a seeded ground-truth pose (synth.depth_images) by default, the pipeline's depth and "
                         "hand_mask under --input-pipeline; needs --test-samples > 0")
    args = ap.parse_args(argv)
    if args.chamfer_w < 0:
        raise SystemExit("--chamfer-w must be >= 0")
    if not args.sil_w >= 0:
        raise SystemExit("--sil-w must be >= 0")
    if args.sil_occluder and not args.sil_w > 0:
        raise SystemExit("--sil-occluder needs --sil-w > 0")
    if args.quant_samples < 0:
        raise SystemExit("--quant-samples must be >= 0")
    from . import ops
    mods = [m.strip() for m in args.mods.split(",") if m.strip()]
    ops.mods_bits(mods)                               # NotImplementedError for anything but uv / xyz, before any work
    cfg = None
    if args.cfg:
        cfg = harness.load_config(args.cfg)
        args.backbone, args.hidden, args.flow_steps = cfg.network.backbone, cfg.network.h_dims[0], cfg.network.num_steps
        args.batch, args.lr, args.milestones = cfg.training.batch_size, cfg.training.lr, list(cfg.training.milestones)
        args.test_samples = cfg.training.get("test_samples", args.test_samples)
    if args.quant_samples > args.test_samples:
        raise SystemExit(f"--quant-samples {args.quant_samples} is more than the {args.test_samples} hypotheses of --test-samples")
    if args.mesh_metrics and not args.test_samples > 0:
        raise SystemExit("--mesh-metrics needs --test-samples > 0 (the meshes come from the metrics pass)")
    if args.pck_metrics and not args.test_samples > 0:
        raise SystemExit("--pck-metrics needs --test-samples > 0 (the joints and meshes come from the metrics pass)")
    if args.depth_metrics and not args.test_samples > 0:
        raise SystemExit("--depth-metrics needs --test-samples > 0 (the meshes come from the metrics pass)")

    rank, local_rank, world, dist = mdist.init()
    if not torch.cuda.is_available():
        raise SystemExit("mhentropy_amd.run needs a HIP device (there is no CPU path)")
    torch.cuda.set_device(local_rank if world > 1 else 0)
    torch.manual_seed(args.seed)                      # same initial weights on every rank
    ops.rng_state(torch.device("cuda", torch.cuda.current_device()), seed=args.seed + 7919 * rank)      # the device generator of the base noise
    cd = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    if cfg is not None:
        from .network import MHEnt
        special, common = harness.mhent_cfgs_from_config(cfg, tables=synth.mano_tables(0), compute_dtype=cd)
        model = MHEnt(special, **common)
        model.q_z_giv_i.compute_dtype = cd
        model = model.cuda().train()
    else:
        model = harness.build_mhent(backbone=args.backbone, h_dims=(args.hidden, args.hidden), num_steps=args.flow_steps,
                                    tables=synth.mano_tables(0), compute_dtype=cd).cuda().train()
    if args.load:
        ck = harness.load_model(args.load, model, map_location="cuda")
        if isinstance(ck, dict) and ck.get("mhe_rng_state") is not None and rank == 0 and world == 1:
            # continue the checkpointed run's base-noise stream (single process; under data parallelism every rank keeps its own seed)
            ops.rng_set_state(torch.device("cuda", torch.cuda.current_device()), ck["mhe_rng_state"])
    scalars = harness.ScalarLog(args.scalars) if (args.scalars and rank == 0) else None
    trainer = TrainStep(model, lr=args.lr, max_norm=1.0, dist=dist)
    criterion = MHEntLoss(aligned=args.aligned)
    meters = {"loss": harness.AverageMeter(), "epe3d": harness.AverageMeter(), "epe2d": harness.AverageMeter()}
    if args.mesh_metrics:
        meters.update({k: harness.AverageMeter() for k in harness.MESH_SCALARS})
    if args.depth_metrics:
        meters.update({k: harness.AverageMeter() for k in harness.DEPTH_SCALARS})
    pck_pool = None
    if args.pck_metrics:
        meters.update({k: harness.AverageMeter() for k in harness.PCK_SCALARS})
        pck_pool = {k: harness.PckPool() for k in harness.PCK_SCALARS[:4]}
    step, log = 0, []
    graphed, graphed_lr, sx, sy = None, None, None, None
    if args.input_pipeline:
        import numpy as np
        from . import ho3d_dataloader as hd
        pipe = hd.HO3DBatchPipeline()
        pool = [synth.ho3d_sample(args.seed + 50 * rank + i, ((i * 37) % 400 - 200, (i * 53) % 300 - 150)) for i in range(8)]
        aug_rng = np.random.RandomState(args.seed + rank)
    for epoch in range(args.epochs):
        trainer.lr = harness.multistep_lr(args.lr, epoch, tuple(args.milestones))
        for m in meters.values():
            m.reset()
        t0 = time.time()
        it_losses = []
        for it in range(args.iters):
            if args.input_pipeline:
                order = aug_rng.randint(0, len(pool), args.batch)
                raw = hd.collate_decoded([pool[i] for i in order])
                x, y = pipe(raw, aug=hd.draw_aug(args.batch, aug_rng))
                if args.chamfer_w > 0:
                    y["object_count"] = raw["obj_count"]
            else:
                xn, yn = synth.batch(args.seed + 1000 * rank + step, args.batch, image_size=args.image_size)
                x = torch.as_tensor(xn).cuda()
                if args.chamfer_w > 0:
                    yn.update(synth.object_targets(args.seed + 1000 * rank + step, args.batch, with_count=True))
                if args.sil_w > 0:
                    yn["hand_mask"] = synth.hand_masks(args.seed + 1000 * rank + step, args.batch, crop_uv=yn["crop_uv"])
                if args.sil_occluder:
                    yn["hand_mask"], yn["object_mask"] = synth.object_masks(args.seed + 1000 * rank + step, yn["hand_mask"])
                y = {k: torch.as_tensor(v).cuda() for k, v in yn.items()}
                if args.mesh_metrics or args.depth_metrics or args.pck_metrics:
                    with torch.no_grad():          # the mesh of the seeded ground-truth pose, normalised like the hypotheses' meshes
                        y["verts"] = model.mano_dec.verts(torch.as_tensor(synth.mesh_pose(args.seed + 1000 * rank + step, args.batch)).cuda())
                if args.depth_metrics:
                    with torch.no_grad():          # ... and its depth crop under the target camera
                        y.update(synth.depth_images(y, model.mano_dec.mano_layer.faces_i32, args.seed + 1000 * rank + step,
                                                    scale=y["scale"] if args.chamfer_w > 0 else None))          # (the object targets' bone length)
            model.training_step_start(step)
            if args.graph and not args.test_samples:
                from .train import GraphedStep
                yk = {k: y[k].contiguous() for k in ("crop_uv", "vis") + (("pose3d",) if "xyz" in mods else ()) +      # what the loss consumes
                      (("object_verts", "object_count", "scale", "original_pose3d") if args.chamfer_w > 0 else ()) +
                      (("hand_mask",) if args.sil_w > 0 else ()) + (("object_mask",) if args.sil_occluder else ())}
                if graphed is None or graphed_lr != trainer.lr:
                    # (re-)capture: GraphedStep's warm-up pass is one real step on this batch - it IS this iteration (replaying the
                    # same batch as well would apply two optimizer steps to it and advance Adam's count and the BatchNorm buffers twice)
                    sx, sy = x.clone(), {k: v.clone() for k, v in yk.items()}
                    graphed, graphed_lr = GraphedStep(trainer, sx, sy, N=args.hyps, mods=mods, chamfer_w=args.chamfer_w, sil_w=args.sil_w,
                                                       sil_occluder=args.sil_occluder), trainer.lr
                    out = graphed.warm_out
                else:
                    sx.copy_(x)
                    for k, v in yk.items():
                        sy[k].copy_(v)
                    out = graphed.replay()
            else:
                out = trainer.step(x, y, N=args.hyps, test_samples=args.test_samples, mods=mods, chamfer_w=args.chamfer_w, sil_w=args.sil_w,
                                   test_quant=args.quant_samples, quant=args.quant, sil_occluder=args.sil_occluder)
            with torch.no_grad():
                total, losses, metrics = criterion(dict(out), y)
            meters["loss"].update(float(total))
            it_losses.append(float(total))
            if scalars is not None:
                scalars.iteration(step, losses, metrics, out)
            if args.mesh_metrics:
                ms = harness.mesh_scalars(out, y)
                for k, v in ms.items():
                    meters[k].update(v)
                if scalars is not None:
                    scalars.mesh(step, ms)
            if args.pck_metrics:
                ps = harness.pck_scalars(out, y, pool=pck_pool)
                for k, v in ps.items():
                    meters[k].update(v)
                if scalars is not None:
                    scalars.named(step, ps)
            if args.depth_metrics:
                with torch.no_grad():
                    ds = harness.depth_scalars(out, y)
                for k, v in ds.items():
                    meters[k].update(v)
                if scalars is not None:
                    scalars.mesh(step, ds)
            if args.test_samples:
                meters["epe3d"].update(float(metrics["eucLoss_3d_rgb_sample"].mean()))
                meters["epe2d"].update(float(metrics["eucLoss_2d_rgb_sample"].mean()))
            step += 1
        torch.cuda.synchronize()
        rec = mdist.reduce_mean_scalars({k: float(m.avg) for k, m in meters.items()}, dist, device=torch.device("cuda"))
        rec.update(epoch=epoch, lr=trainer.lr, img_per_s=round(world * args.batch * args.iters / (time.time() - t0), 1),
                   it_losses=[round(v, 4) for v in it_losses])          # this rank's per-iteration totals (the resume test reads the first)
        log.append(rec)
        if scalars is not None:
            scalars.epoch(step, rec["loss"], rec["epe3d"])
        if rank == 0:
            print(json.dumps(rec), flush=True)
    if pck_pool is not None and rank == 0:          # this rank's pooled curves of the top hypothesis over every iteration of the run
        print(json.dumps({"pck_pooled_auc": {k: round(p.auc(), 6) for k, p in pck_pool.items()}}), flush=True)
    if scalars is not None:
        scalars.close()
    if args.save and rank == 0:
        harness.save_model(args.save, model, rng_words=ops.rng_get_state(torch.device("cuda", torch.cuda.current_device())))
    if dist is not None:
        dist.destroy_process_group()
    main.last_trainer = trainer           # (tests: optimizer step count, parameters)
    main.last_pck_pool = pck_pool         # (tests: the pooled curves)
    return log


if __name__ == "__main__":
    main(sys.argv[1:])
