"""The fused fields' weight packers (dnerf_amd/fused.py `pack_weights`, dnerf_amd/fused_f32.py `pack_weights_f32` and
`pack_weights_f32_split`) are numpy over the model's weights plus the library's two size getters: no GPU needed.

The digests below pin the byte layout the kernels read.  They were recorded with this file's `_stub_model` from the packers as they
stood BEFORE the twelve-entry layer plan was shared between `pack_weights` and `pack_weights_f32_split` (a checkout of the parent
commit of that change, not the code under test), so a packer that changes a byte, a dtype or a shape fails here."""
import hashlib
import types

import numpy as np
import pytest
import torch

_SHAPES = dict(deform_net=[(128, 76)] + [(128, 128)] * 6 + [(3, 128)], sigma_net=[(64, 32), (16, 64)], color_net=[(64, 31), (64, 64), (3, 64)])

_PINNED = {
    "pack_weights": ("float16", (240, 64, 8), "e0b03bfd63d035e02f95368ab15a2213f71aa9005589ab95a5db3a45283db406"),
    "pack_weights_f32": ("float32", (122880,), "2a44a8cce200e83394596595d6a37caca87d2b96956b97a64d772fd0c23f4670"),
    "pack_weights_f32_split": ("uint16", (245760,), "b3768bedd0e2da4660470823c85d07bdb4fac614253d05f8d0549806362bebf0"),
}


def _stub_model():
    """Thirteen `.weight` tensors from a closed form without RNG and without libm: an integer pattern divided by a prime (one correctly
    rounded division, then one rounding to float32), so every platform builds the same bits; the quotients are not fp16 values, so the
    split packer's lo halves are exercised."""
    m, k = types.SimpleNamespace(), 0
    for name, shapes in _SHAPES.items():
        layers = []
        for out_dim, in_dim in shapes:
            r, c = np.arange(out_dim, dtype=np.int64)[:, None], np.arange(in_dim, dtype=np.int64)[None, :]
            w = (((r * 131 + c * 71 + r * c * 7 + k * 13) % 1009 - 504) / 1013.0).astype(np.float32)
            layers.append(types.SimpleNamespace(weight=torch.from_numpy(w)))
            k += 1
        setattr(m, name, layers)
    return m


@pytest.mark.parametrize("name", sorted(_PINNED))
def test_packed_weights_keep_their_bytes(name):
    from dnerf_amd import fused, fused_f32
    packed = getattr(fused if name == "pack_weights" else fused_f32, name)(_stub_model())
    dtype, shape, digest = _PINNED[name]
    assert str(packed.dtype) == dtype and packed.shape == shape
    assert hashlib.sha256(np.ascontiguousarray(packed).tobytes()).hexdigest() == digest
