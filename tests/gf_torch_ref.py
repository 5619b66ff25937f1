"""A second zfec reference, for blocks too large for oracle/fec_oracle.c -- TEST INFRASTRUCTURE ONLY.

Plain torch on whichever device its tensors live on: a row of a GF(2^8) matrix product is the XOR of
table gathers MUL[c][block].  Everything it knows about the code comes from oracle/zfec_ref.py (the
multiplication table MUL and the matrices encode_matrix / parity_rows / decode_matrix); nothing comes
from the product's headers or from the library.  tests/test_gf_torch_ref.py ties it byte for byte to
the C oracle (oracle/fec_oracle.c via cfec) at small sizes; the GPU tests of large blocks
(tests/test_gpu_large_blocks.py) rest on that link.
"""

from __future__ import annotations

import numpy as np
import torch

from oracle import zfec_ref

_MUL = {}


def mul_table(device) -> torch.Tensor:
    """zfec_ref.MUL as a [256, 256] uint8 tensor on `device`."""
    device = torch.device(device)
    if device not in _MUL:
        _MUL[device] = torch.from_numpy(np.ascontiguousarray(zfec_ref.MUL)).to(device)
    return _MUL[device]


def rows(coef, blocks: torch.Tensor) -> torch.Tensor:
    """coef: uint8 [r, c] (numpy or tensor); blocks: uint8 tensor [c, B].  -> uint8 [r, B], row i the
    XOR over j of MUL[coef[i, j]][blocks[j]]."""
    coef = torch.as_tensor(np.ascontiguousarray(coef) if isinstance(coef, np.ndarray) else coef)
    assert coef.dtype == torch.uint8 and blocks.dtype == torch.uint8
    assert coef.dim() == 2 and blocks.dim() == 2 and coef.shape[1] == blocks.shape[0], (coef.shape, blocks.shape)
    mul = mul_table(blocks.device)
    coef = coef.to(blocks.device).long()
    out = torch.zeros((coef.shape[0], blocks.shape[1]), dtype=torch.uint8, device=blocks.device)
    for j in range(blocks.shape[0]):
        tab = mul[coef[:, j]]  # [r, 256]: row i the multiples of coef[i, j]
        out ^= torch.index_select(tab, 1, blocks[j].long())
    return out


def split(chunk: torch.Tensor, k: int) -> torch.Tensor:
    """easyfec's split: k blocks of B = ceil(n / k) bytes as [k, B], block k-1 zero padded.  zfec
    refuses a chunk whose padding would not fit in block k-1 (blocks of unequal length)."""
    n = chunk.numel()
    B = -(-n // k)
    if k > 1 and (k - 1) * B > n:
        raise ValueError("Precondition violation: Input blocks are required to be all the same length.")
    data = torch.zeros(k * B, dtype=torch.uint8, device=chunk.device)
    data[:n] = chunk
    return data.view(k, B)


def encode(chunk: torch.Tensor, k: int, m: int) -> torch.Tensor:
    """All m blocks of a chunk (uint8, 1-D) as [m, B]: the k data blocks, then the m - k parity rows."""
    assert chunk.dtype == torch.uint8 and chunk.dim() == 1
    data = split(chunk, k)
    if m == k:
        return data
    return torch.cat([data, rows(zfec_ref.parity_rows(k, m), data)])
