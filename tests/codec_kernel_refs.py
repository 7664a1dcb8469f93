"""fp64 references of the Code2Wav kernels (csrc/codec.hip, csrc/conv_unit.hip), one per kernel, each a restatement of the
formula in the kernel's header comment in plain torch on the CPU -- TEST INFRASTRUCTURE.  None follows the kernel's code: no
chunks, no online softmax, no tiles.  Inputs are the bf16 / fp32 values a test uploads, widened exactly to fp64, so the rounding
of an input is never counted as kernel error.  Activations are time-major [T, C] like the kernels'.
PINNED: tests/test_codec_kernel_refs.py holds every function here to oracle/code2wav_oracle.py (itself pinned to the reference
module's outputs) and, where the oracle's configurations do not reach (GQA, head_dim 128), to a literal loop."""
from __future__ import annotations

import torch

F64 = torch.float64


def _d(x: torch.Tensor) -> torch.Tensor:
    return x.detach().cpu().to(F64)


def bf16_round(x: torch.Tensor) -> torch.Tensor:
    """fp64 -> the nearest bf16 value (ties to even), as fp64."""
    return x.to(torch.bfloat16).to(F64)


def ref_rvq_embed(codes: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
    """codes long [Q, T], table [Q, bins, C] -> [T, C]: sum over the quantizers of table[q][clamp(codes[q, t], 0, bins - 1)]."""
    Q, bins, _ = table.shape
    idx = codes.detach().cpu().long().clamp(0, bins - 1)
    return _d(table)[torch.arange(Q)[:, None], idx].sum(0)


def ref_rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float) -> torch.Tensor:
    """x [T, H] -> w * x / sqrt(mean(x^2) + eps)."""
    x = _d(x)
    return _d(w) * (x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def rope_angles(T: int, hd: int, theta: float) -> torch.Tensor:
    """angle(t, d) = t * theta^(-2 d / hd), d < hd / 2, in fp64: [T, hd / 2]."""
    inv = torch.tensor(float(theta), dtype=F64) ** (-torch.arange(0, hd, 2, dtype=F64) / hd)
    return torch.arange(T, dtype=F64)[:, None] * inv[None]


def rotate_half(qkv: torch.Tensor, heads: int, hd: int, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    """The first `heads` heads of each row: (x1, x2) = (x[d], x[d + hd/2]) -> (x1 cos - x2 sin, x2 cos + x1 sin); cos / sin
    [T, hd / 2].  Everything behind those heads is returned unchanged."""
    out = _d(qkv).clone()
    T, half = out.shape[0], hd // 2
    x = out[:, :heads * hd].reshape(T, heads, 2, half)
    x1, x2 = x[:, :, 0], x[:, :, 1]
    c, s = cos.to(F64)[:, None, :], sin.to(F64)[:, None, :]
    out[:, :heads * hd] = torch.stack([x1 * c - x2 * s, x2 * c + x1 * s], 2).reshape(T, heads * hd)
    return out


def ref_rope(qkv: torch.Tensor, q_heads: int, kv_heads: int, hd: int, theta: float) -> torch.Tensor:
    """qkv [T, ld], row = [q heads | k heads | v heads | pad]: rotate-half RoPE on the q and k heads, position = row index.
    v heads and pad columns are returned unchanged."""
    ang = rope_angles(qkv.shape[0], hd, theta)
    return rotate_half(qkv, q_heads + kv_heads, hd, ang.cos(), ang.sin())


def ref_window_attn(qkv: torch.Tensor, nh: int, nkv: int, hd: int, window: int, scale: float) -> torch.Tensor:
    """qkv [T, ld], row = [q heads | k heads | v heads | pad] (already rotated) -> [T, nh * hd]: for query t the keys j with
    0 <= t - j < window, query head h on kv head h // (nh // nkv), softmax of scale * q . k over those keys."""
    x = _d(qkv)
    T = x.shape[0]
    q = x[:, :nh * hd].reshape(T, nh, hd)
    k = x[:, nh * hd:(nh + nkv) * hd].reshape(T, nkv, hd)
    v = x[:, (nh + nkv) * hd:(nh + 2 * nkv) * hd].reshape(T, nkv, hd)
    kvh = torch.arange(nh) // (nh // nkv)
    s = torch.einsum("thd,jhd->htj", q, k[:, kvh]) * scale
    t, j = torch.arange(T)[:, None], torch.arange(T)[None]
    s = s.masked_fill(~((t - j >= 0) & (t - j < window)), float("-inf"))
    return torch.einsum("htj,jhd->thd", torch.softmax(s, -1), v[:, kvh]).reshape(T, nh * hd)


def causal_taps(x: torch.Tensor, taps: int, dilation: int = 1) -> torch.Tensor:
    """x [T, C] -> [taps, T, C]: tap j of row t is x[t - (taps - 1 - j) * dilation], zero where that row is before t = 0."""
    T = x.shape[0]
    pad = torch.cat([x.new_zeros((taps - 1) * dilation, x.shape[1]), x], 0)
    return torch.stack([pad[j * dilation:j * dilation + T] for j in range(taps)], 0)


def ref_dwconv_ln(x, w, b, ln_w, ln_b, eps: float, taps: int, parts: bool = False):
    """x [T, C], w [C, taps]: y[t, c] = b[c] + sum_j w[c][j] x[t - (taps - 1) + j][c] with zero rows before t = 0, then
    LayerNorm over the channels (biased variance) * ln_w + ln_b.  parts=True adds what the test's tolerance is made of."""
    xt = causal_taps(_d(x), taps)                                            # [taps, T, C]
    prod = xt * _d(w).T[:, None, :]
    y = prod.sum(0) + _d(b)
    mean = y.mean(-1, keepdim=True)
    rstd = torch.rsqrt((y - mean).pow(2).mean(-1, keepdim=True) + eps)
    n = (y - mean) * rstd
    out = n * _d(ln_w) + _d(ln_b)
    if parts:
        return out, dict(n=n, rstd=rstd, abs_sum=prod.abs().sum(0) + _d(b).abs())
    return out


def ref_out_conv(x, w, bias: float, taps: int, parts: bool = False):
    """x [T, C], w [taps, C]: wav[t] = clamp(bias + sum_{j, c} w[j][c] x[t - (taps - 1) + j][c], -1, 1), zero rows before t = 0."""
    prod = causal_taps(_d(x), taps) * _d(w)[:, None, :]
    raw = prod.sum((0, 2)) + float(bias)
    if parts:
        return raw.clamp(-1.0, 1.0), dict(raw=raw, abs_sum=prod.abs().sum((0, 2)) + abs(float(bias)))
    return raw.clamp(-1.0, 1.0)


def snake_params(alpha: torch.Tensor, beta: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """SnakeBeta's per-channel parameters as the decoder uploads them (code2wav.py::_build): fp32 (exp(alpha), 1 / (exp(beta) + 1e-9))."""
    a, b = alpha.detach().float().cpu(), beta.detach().float().cpu()
    return torch.exp(a), 1.0 / (torch.exp(b) + 1e-9)


def ref_snake(x: torch.Tensor, sn: tuple[torch.Tensor, torch.Tensor]) -> torch.Tensor:
    """x + 1 / (exp(beta) + 1e-9) * sin^2(x * exp(alpha)) per channel; sn = snake_params(alpha, beta), widened to fp64."""
    return x + _d(sn[1]) * torch.sin(x * _d(sn[0])) ** 2


def ref_res_unit(s, h, W1, b1, snake2, W2, b2, snake_next, dilation: int, bf16: bool = True, parts: bool = False):
    """One residual unit: h_new = h + conv1x1(snake2(conv7_dilated(s))), s_next = snake_next(h_new).
    s [T, C] (bf16 values), h [T, C] fp32, W1 [C, C, 7] / W2 [C, C, 1] in Conv1d layout [out, in, tap] (bf16 values), snake2 /
    snake_next = snake_params(alpha, beta).  bf16=True rounds to bf16 at the kernel's two rounding points: the 1x1 conv's
    operand (after snake2) and s_next; everything else is fp64.  Returns (h_new, s_next)."""
    s, W1, W2 = _d(s), _d(W1), _d(W2)[:, :, 0]
    xt = causal_taps(s, W1.shape[2], dilation)                               # [7, T, C]
    y1 = torch.einsum("jtc,ncj->tn", xt, W1) + _d(b1)
    u_exact = ref_snake(y1, snake2)
    u = bf16_round(u_exact) if bf16 else u_exact
    h_new = _d(h) + u @ W2.T + _d(b2)
    s_exact = ref_snake(h_new, snake_next)
    s_next = bf16_round(s_exact) if bf16 else s_exact
    if parts:
        abs1 = torch.einsum("jtc,ncj->tn", xt.abs(), W1.abs()) + _d(b1).abs()
        return h_new, s_next, dict(y1=y1, u=u, abs1=abs1)
    return h_new, s_next
