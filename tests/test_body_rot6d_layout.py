"""Host-only checks of body.rotmat_to_rot6d, the re-arrangement BodyFlowHead.log_prob applies to annotated rotations: the 6D pose is the first two
COLUMNS of the rotation, the layout the reference's compute_rotation_matrix_from_ortho6d reads (hand/manopth/rot6d.py:12-23)."""
import numpy as np
import pytest
import torch

from mhentropy_amd import body


def test_rotmat_to_rot6d_is_the_first_two_columns():
    M = torch.arange(2 * 24 * 9, dtype=torch.float32).view(2, 24, 3, 3)
    p = body.rotmat_to_rot6d(M)
    assert p.shape == (2, 24, 6) and p.dtype == M.dtype
    assert torch.equal(p[..., :3], M[..., :, 0]) and torch.equal(p[..., 3:], M[..., :, 1])
    assert torch.equal(body.rotmat_to_rot6d(M[0, 0]), torch.tensor([0., 3., 6., 1., 4., 7.]))


def test_rotmat_to_rot6d_inverts_the_oracle_rotation():
    """rotation_from_ortho6d(rotmat_to_rot6d(R)) == R for rotations R made by the oracle from random 6D (float64: 1e-12)"""
    from oracle import rot6d_ref
    M = rot6d_ref.rotation_from_ortho6d(torch.as_tensor(np.random.default_rng(0).normal(0, 1, (40, 6))))
    back = rot6d_ref.rotation_from_ortho6d(body.rotmat_to_rot6d(M))
    assert float((back - M).abs().max()) <= 1e-12


def test_rotmat_to_rot6d_refuses_other_shapes():
    with pytest.raises(ValueError):
        body.rotmat_to_rot6d(torch.zeros(4, 9))
