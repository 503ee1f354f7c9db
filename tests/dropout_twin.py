"""Twin of the dropout kernels  --  TEST INFRASTRUCTURE ONLY.

  * Philox4x32-10 (Salmon et al., SC'11; the Random123 constants) in NumPy and the mask rule of include/easyhybrid_hip.h:
    key = (seed lo, seed hi), counter = (k, 32 l + (u >> 2), step lo, step hi), unit u kept iff word (u & 3) >= T,
    T = min(2^32 - 1, floor(p 2^32)) with p the float32 rate the C ABI takes, compared unsigned.
  * the feed-forward hybrid model's forward / loss / gradient in torch (fp64 or fp32) with EXPLICIT masks: the output of hidden layer l is
    act(z) * mask_l * invp_l, invp = 1 / (1 - p) in fp32 (one multiplication by a pre-scaled mask, as Lux's dropout does).  The
    mechanistic models and the activations are oracle/torch_twin.py's."""
import numpy as np
import torch

from oracle import torch_twin as tt

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """four counter words (arrays broadcast together), two key words -> four output words (uint32 arrays)"""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, np.uint32) for c in (c0, c1, c2, c3)])
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = c0.astype(np.uint64) * M0, c2.astype(np.uint64) * M1
        hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), p0.astype(np.uint32)
        hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), p1.astype(np.uint32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint32(k0), lo1, hi0 ^ c3 ^ np.uint32(k1), lo0
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def threshold(p) -> int:
    return min(0xFFFFFFFF, int(np.floor(float(np.float32(p)) * 4294967296.0)))


def invp(p) -> np.float32:
    return np.float32(1) / (np.float32(1) - np.float32(p))


def keep_mask(seed: int, step: int, count: int, layer: int, width: int, p) -> np.ndarray:
    """(count, width) bool: unit u of hidden layer `layer` of the k-th sample of the minibatch is kept at training step `step`"""
    k = np.arange(count, dtype=np.uint32)[:, None]
    q = np.arange((width + 3) // 4, dtype=np.uint32)[None, :] + np.uint32(32 * layer)
    w = philox4x32_10(k, q, np.uint32(step & 0xFFFFFFFF), np.uint32((step >> 32) & 0xFFFFFFFF), seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u = np.stack(w, axis=-1).reshape(count, -1)[:, :width]
    return u >= np.uint32(threshold(p))


def masks_for(seed, step, count, hidden, rates):
    """per hidden layer: the (count, width) keep mask, or None where the rate is 0"""
    return [keep_mask(seed, step, count, l, w, p) if p > 0 else None for l, (w, p) in enumerate(zip(hidden, rates))]


def forward(spec, theta, X, forcings, masks=None, scales=None):
    """oracle.torch_twin.forward for one fp32 network, with masks[l] (count, width) and scales[l] on hidden layer l (None: none)"""
    assert spec.nets is None and getattr(spec, "precision", "f32") == "f32"
    dt = theta.dtype
    h = torch.as_tensor(X, dtype=dt)
    if getattr(spec, "input_batchnorm", False):            # train-mode batch statistics, biased variance, eps = 1e-5
        h = (h - h.mean(dim=1, keepdim=True)) / torch.sqrt(h.var(dim=1, unbiased=False, keepdim=True) + 1e-5)
    off, dims = 0, spec.layer_dims
    for li, (o, i) in enumerate(dims):
        W = theta[off:off + o * i].reshape(i, o).T
        off += o * i
        b = theta[off:off + o]
        off += o
        z = W @ h + b[:, None]
        if li == len(dims) - 1:
            h = z
        else:
            h = tt._act(spec.act_of(0, li), z)
            if masks is not None and masks[li] is not None:
                m = torch.as_tensor(np.ascontiguousarray(masks[li].T), dtype=dt) * float(scales[li])
                h = h * m
    par = {}
    for k, n in enumerate(spec.neural):
        par[n] = (spec.lo(n) + (spec.hi(n) - spec.lo(n)) * torch.sigmoid(h[k])) if spec.scale_nn_outputs else h[k]
    for j, g in enumerate(spec.glob):
        par[g] = spec.lo(g) + (spec.hi(g) - spec.lo(g)) * torch.sigmoid(theta[off + j:off + j + 1])
    for f in spec.fixed:
        par[f] = torch.full((1,), spec.default(f), dtype=dt)
    frc = {k: torch.as_tensor(v, dtype=dt) for k, v in forcings.items()}
    return tt._mech(spec, par, frc)


def loss_and_grad(spec, theta_np, X, forcings, targets, masks=None, scales=None, dtype=torch.float64):
    """mse (sum over the targets of the mean over their valid samples) and its gradient; (loss, grad, n valid)"""
    theta = torch.tensor(np.asarray(theta_np), dtype=dtype, requires_grad=True)
    out = forward(spec, theta, X, forcings, masks, scales)
    tot, nv = 0, 0
    for t in spec.targets:
        y = torch.as_tensor(targets[t], dtype=dtype)
        m = ~torch.isnan(y)
        if int(m.sum()) == 0:
            continue
        nv += int(m.sum())
        tot = tot + torch.mean((out[t][m] - y[m]) ** 2)
    if not torch.is_tensor(tot):
        return 0.0, np.zeros(theta.numel()), 0
    tot.backward()
    return float(tot.detach()), theta.grad.numpy().copy(), nv
