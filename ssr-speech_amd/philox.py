"""Host replica of the device-side sampling-noise stream (csrc/noise.hip, DESIGN.md Part I.21). Pure numpy; used by tests and tools only —
the product path never needs it.

The stream: Philox4x32-10, key = the utterance's seed as an unsigned 64-bit value (low word, high word), counter = (b, t, TAG, 0) with t
the step within the utterance and b the block; word j of block b is element e = 4b + j of the step's flattened [K, card] tensor. A word w
gives n = w >> 9, u = (n + 0.5) * 2^-23 — exact in fp32: (2n + 1) * 2^-24 has at most 24 significant bits — and the value q = -log(u).
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the key increments
TAG = 0x6E6F6973                         # counter word 2: "nois"
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key) -> np.ndarray:
    """counter [..., 4], key [..., 2] (broadcast against each other; any integer type, taken mod 2^32) -> the output block [..., 4] uint32."""
    c = np.asarray(counter).astype(np.uint64) & _MASK
    k = np.asarray(key).astype(np.uint64) & _MASK
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], lead) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], lead) for i in range(2))
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _MASK, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _MASK
        k0, k1 = (k0 + np.uint64(W0)) & _MASK, (k1 + np.uint64(W1)) & _MASK
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def seed_key(seed: int):
    """(low word, high word) of the seed as an unsigned 64-bit value — what `DecodeKnobs.seed` becomes in the sampler record."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    return s & 0xFFFFFFFF, s >> 32


def words(seed: int, first_step: int, n_steps: int, K: int, card: int) -> np.ndarray:
    """The raw words of steps [first_step, first_step + n_steps): uint32 [n_steps, K, card]."""
    kc = int(K) * int(card)
    nb = (kc + 3) // 4
    ctr = np.zeros((int(n_steps), nb, 4), dtype=np.uint64)
    ctr[..., 0] = np.arange(nb, dtype=np.uint64)[None, :]
    ctr[..., 1] = (np.arange(int(n_steps), dtype=np.uint64) + np.uint64(first_step))[:, None]
    ctr[..., 2] = TAG
    out = philox4x32_10(ctr, np.asarray(seed_key(seed), dtype=np.uint64))
    return out.reshape(int(n_steps), nb * 4)[:, :kc].reshape(int(n_steps), int(K), int(card))


def uniforms(w: np.ndarray) -> np.ndarray:
    """u = ((w >> 9) + 0.5) * 2^-23 as float64 (exact, and exactly representable in fp32)."""
    return ((np.asarray(w, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def exp_noise(seed: int, first_step: int, n_steps: int, K: int, card: int) -> np.ndarray:
    """The Exp(1) draws of steps [first_step, first_step + n_steps) of the utterance with this seed: float64 [n_steps, K, card], -log of the
    exact u. `exp_noise32` is the fp32 view (what the device's -logf(u) is compared with)."""
    return -np.log(uniforms(words(seed, first_step, n_steps, K, card)))


def exp_noise32(seed: int, first_step: int, n_steps: int, K: int, card: int) -> np.ndarray:
    return exp_noise(seed, first_step, n_steps, K, card).astype(np.float32)
