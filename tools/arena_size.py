"""Elements of the train step's derived-operand arenas at ResNet-50 bf16, against the parameter count."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mhentropy_amd import harness, synth
from mhentropy_amd.train import TrainStep
model = harness.build_mhent(backbone="resnet50", tables=synth.mano_tables(0), compute_dtype=torch.bfloat16).cuda().train()
ar = TrainStep(model).arena
for dt, a in ar.main.items():
    print(dt, a.used / 1e6, "M elements; params", ar.n_params / 1e6)
