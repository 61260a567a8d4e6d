import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from mhentropy_amd import harness, synth
from mhentropy_amd.train import TrainStep
B, K = 256, 64
model = harness.build_mhent(backbone="resnet50", tables=synth.mano_tables(0), compute_dtype=torch.bfloat16, flow="glow").cuda().train()
x, yn = synth.batch(0, B, image_size=256)
x = torch.as_tensor(x).cuda(); y = {k: torch.as_tensor(v).cuda() for k, v in yn.items()}
noise = torch.as_tensor(synth.noise(0, K * B)).cuda()
ts = TrainStep(model)
def T(f, n=3):
    f(); torch.cuda.synchronize(); t0 = time.time()
    for _ in range(n): f()
    torch.cuda.synchronize(); return (time.time() - t0) / n * 1e3
print("forward", T(lambda: ts.forward(x, y, noise=noise, N=K)))
print("fwd+bwd", T(lambda: ts.forward_backward(x, y, noise=noise, N=K)))
print("opt", T(lambda: ts.optimizer_step()))
ts.forward(x, y, noise=noise, N=K)
feat = ts.tape["feat"]
print("glow fwd", T(lambda: ts.glow.forward(noise, feat)))
g45 = torch.randn(K * B, 45, device="cuda"); gl = torch.full((B,), -1.0 / B, device="cuda")
ts.raw.zero_()
print("glow bwd", T(lambda: ts.glow.backward(g45, gl, K, B)))
print("reparam", T(lambda: ts.glow._reparam_backward(gl)))
print("pack", T(lambda: ts.glow._pack()))
