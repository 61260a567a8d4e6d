"""MHEntLoss with the reference's call surface (reference hand/criteria.py:42-173):
`MHEntLoss(loss_weights, aligned)(output, target) -> (total, losses, metrics)`; the metrics
block runs in one HIP kernel (csrc/metrics.hip), the Procrustes alignment of the aligned
evaluation in csrc/procrustes.hip."""
import torch
from torch import nn

from . import ops

# row order of mhe_metrics_f32's [14,B] output
METRIC_KEYS = tuple(f"eucLoss_{sup}_rgb_{row}" for sup in ("3d", "2d")
                    for row in ("sample", "sample_std", "vis", "vis_std", "vis_mean", "invis", "invis_std"))


class MHEntLoss(nn.Module):
    def __init__(self, loss_weights=None, aligned=False):
        """aligned: the reference's evaluation branch (criteria.py:62-87) - every hypothesis' joints and mesh are Procrustes-aligned
        with scale to target['pose3d'] / target['verts'] (a label whose target is absent is left as it is); output['xyz'] and
        output['verts'] are replaced by new aligned tensors.  The 3D error rows are taken of the aligned joints, the 3D spread rows
        of the unaligned ones (criteria.py:63-68,141), the 2D rows are unchanged."""
        super().__init__()
        self.loss_weights = loss_weights
        self.aligned = aligned

    def forward(self, output, target):
        losses = {"neg_log_p": -output["log_p"]}          # criteria.py:55
        metrics = {}
        unaligned_xyz = output.get("xyz")
        if self.aligned:
            for lbl in ("xyz", "verts"):
                tgt = target["pose3d"] if lbl == "xyz" else target.get("verts")
                if lbl in output and tgt is not None:
                    output[lbl] = ops.procrustes_align(output[lbl].contiguous(), tgt.contiguous())
        if "xyz" in output:
            if "uv" not in output:
                raise NotImplementedError("uv from ground-truth s,t (criteria.py:100-104) is not on the MHEnt path")
            rest = (output["uv"].contiguous(), target["pose3d"].contiguous(), target["scale"].contiguous(), target["crop_uv"].contiguous(),
                    target["vis"].contiguous())
            if output["xyz"] is unaligned_xyz:
                m = ops.metrics(output["xyz"].contiguous(), *rest)
            else:
                m = ops.metrics_split(output["xyz"], unaligned_xyz.contiguous(), *rest)
            metrics = {k: m[i] for i, k in enumerate(METRIC_KEYS)}
        return sum(v.mean() for v in losses.values()), losses, metrics
