"""Shared checkers for the parity tests."""
import numpy as np


def assert_topk_equivalent(D_ref, I_ref, D, I, tol=1e-3, k=None):
    """Ranked lists must agree up to permutations inside runs of reference scores
    closer than ``tol`` (SURVEY.md §7 hard part 1: even two fp32 summation orders
    reorder such pairs; FAISS's tie order is unspecified).  Scores must agree to
    ``tol``.  The last run may be cut by the top-k boundary, so there only
    score agreement is required."""
    D_ref, I_ref, D, I = (np.asarray(x) for x in (D_ref, I_ref, D, I))
    k = k or D_ref.shape[1]
    assert D.shape[1] >= k and I.shape[1] >= k
    for q in range(D_ref.shape[0]):
        dr, ir, d, i = D_ref[q, :k], I_ref[q, :k], D[q, :k], I[q, :k]
        np.testing.assert_allclose(d, dr, rtol=0, atol=tol * max(1.0, np.abs(dr).max()),
                                   err_msg="scores of query %d" % q)
        start = 0
        while start < k:
            end = start + 1
            while end < k and abs(dr[end - 1] - dr[end]) < tol:
                end += 1
            if end < k:  # closed run: id sets must match
                assert sorted(ir[start:end].tolist()) == sorted(i[start:end].tolist()), \
                    "query %d ranks %d..%d: %s vs %s" % (q, start, end, ir[start:end], i[start:end])
            start = end


def cosine(a, b):
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return (a * b).sum(-1) / np.sqrt((a * a).sum(-1) * (b * b).sum(-1))


# ---- measured margins -------------------------------------------------------------------------------------------
# Every tolerance in the GPU parity tests is meant to sit at ~3x the value measured on an MI355X.  `margin(name, value,
# bar)` asserts value <= bar (or >= for `higher=True`) and records the pair; the session writes them to
# gpurun_out/margins.json (tests/conftest.py), which is how the bars in the test files were set and are re-checked.
MARGINS = {}


def margin(name, value, bar, higher=False):
    value = float(value)
    MARGINS[name] = {"measured": value, "bar": float(bar), "higher_is_better": bool(higher)}
    if higher:
        assert value >= bar, "%s: measured %.6g, bar >= %.6g" % (name, value, bar)
    else:
        assert value <= bar, "%s: measured %.6g, bar <= %.6g" % (name, value, bar)


def trained_like_(model, seed=0, outlier_dims=(77, 588, 391), outlier_value=(-40.0, 60.0, 25.0), diag_heads=6, diag_scale=8.0,
                  qk_std=0.03, dense_std=0.04, norm_gain=2.2, bias_std=0.02):
    """Overwrite a roberta-base-shape model's N(0, 0.02) initialisation (models.py:25-30) with the statistics TRAINED
    checkpoints show -- what the reference actually loads (utils/util.py:241-280); no checkpoint is reachable offline.
      * MASSIVE ACTIVATIONS: in every LayerNorm of the encoder `outlier_dims` carry a bias of `outlier_value` (-40 / 60 / 25,
        gain 0.2) while the other 765 coordinates have gain ~ N(norm_gain, 15 %) -- norm_gain = the standard deviation the
        three outliers give a row, so the ordinary coordinates keep rms ~1.5 through all 12 layers: the bf16 residual
        stream holds values 20-40x its neighbours, and every rounding of one reaches the next GEMM with an absolute error
        tens of times a normal coordinate's.  As in trained models, the dense layers that READ the hidden state weigh
        those three columns down (x 0.02): a network that lets three constants swamp its input is input-independent
        (measured while building this: pairwise cosine of different passages 0.99999999 -- a parity test of nothing).
      * HEAVY TAILS: Student-t (3 degrees of freedom) word embeddings, std ~0.05.
      * SATURATED SOFTMAX with margins: in the first `diag_heads` heads of every layer the key projection is `diag_scale` x
        the query projection, so a token's own key wins by tens of logits (diagonal heads; logits ~ +-100, probabilities
        exactly 1 and ~e^-40); the other heads stay soft (q / k std `qk_std`).  Random q / k weights LARGE enough to
        saturate instead (std 0.09-0.12) make a CHAOTIC function -- near-ties between unrelated keys flip under any
        rounding: the bf16-emulating oracle is then 0.13 (1 - cos) from the fp32 one, fp32 Q / K / P or not -- and at
        diag_scale 16 (logits ~ +-200) the network's sensitivity lifts ANY bf16 activation storage to 1.4e-3 .. 2.3e-3.
      * dense weights std `dense_std` (twice the initialisation), biases N(0, `bias_std`).
    In place, deterministic in `seed`; returns the model."""
    import torch
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("word_embeddings.weight"):
                z = torch.randn(p.shape, generator=g)
                chi = torch.randn((3,) + tuple(p.shape), generator=g).pow(2).sum(0) / 3.0
                p.copy_(0.03 * z / chi.sqrt())                       # t_3: std = sqrt(3) x 0.03
            elif n.endswith("position_embeddings.weight") or n.endswith("token_type_embeddings.weight"):
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
            elif "LayerNorm.weight" in n:
                w = norm_gain * (1.0 + 0.15 * torch.randn(p.shape, generator=g))
                for d in outlier_dims:
                    w[d] = 0.2
                p.copy_(w)
            elif "LayerNorm.bias" in n:
                b = bias_std * torch.randn(p.shape, generator=g)
                for d, a in zip(outlier_dims, outlier_value):
                    b[d] = a
                p.copy_(b)
            elif n == "norm.weight":
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            elif n.endswith("bias"):
                p.copy_(bias_std * torch.randn(p.shape, generator=g))
            elif p.dim() == 2:
                std = qk_std if (".query.weight" in n or ".key.weight" in n) else dense_std
                w = std * torch.randn(p.shape, generator=g)
                if any(t in n for t in (".query.weight", ".key.weight", ".value.weight", "intermediate.dense.weight",
                                        "embeddingHead.weight")):
                    for d in outlier_dims:
                        w[:, d] *= 0.02
                p.copy_(w)
        sd = dict(model.named_parameters())
        for n, p in sd.items():
            if n.endswith("attention.self.key.weight"):
                q = sd[n.replace(".key.", ".query.")]
                rows = diag_heads * (p.shape[0] // model.config.num_attention_heads)
                p[:rows] = diag_scale * q[:rows]
    return model


# ---- scratch-memory fills ---------------------------------------------------------------------------------------
# tests/test_stale_memory_gpu.py: "same inputs, other garbage in the scratch memory -> identical bits out".
FILLS = ("Z", "N", "R")        # zeros (the baseline), bytes 0xFF (NaN as bf16 / fp16 / fp32, -1 as an integer), seeded random bytes


def fill_bytes(t, kind, seed=0):
    """Overwrite every byte of the contiguous tensor `t` (any dtype, any device) with fill `kind`."""
    import torch
    assert t.is_contiguous()
    b = t.reshape(-1).view(torch.uint8)
    if kind == "Z":
        b.zero_()
    elif kind == "N":
        b.fill_(0xFF)
    elif kind == "R":
        g = torch.Generator(device=b.device).manual_seed(seed)
        b.copy_(torch.randint(0, 256, (b.numel(),), generator=g, dtype=torch.uint8, device=b.device))
    else:
        raise ValueError(kind)
    return t


def assert_fills_agree(runs, what=""):
    """runs: {fill: (outputs, filled_ptrs, used_ptrs)} with outputs = {name: tensor}; "Z" must be there.
    * every run used the buffers it filled (the host re-allocates a buffer that is too small: a fill of a buffer the
      host then drops tests nothing),
    * the Z outputs are finite,
    * every output of every other fill is bit-identical to the Z run's (torch.equal: a NaN never compares equal)."""
    import torch
    assert "Z" in runs, "%s: no baseline run" % what
    for f, (out, filled, used) in runs.items():
        assert filled == used, "%s: fill %s went to a buffer the call did not use (%s vs %s)" % (what, f, filled, used)
    ref = runs["Z"][0]
    assert ref, "%s: no outputs" % what
    for n, t in ref.items():
        if t.dtype.is_floating_point:
            assert bool(torch.isfinite(t).all()), "%s: %s is not finite under fill Z" % (what, n)
    for f, (out, _, _) in runs.items():
        if f == "Z":
            continue
        assert sorted(out) == sorted(ref), "%s: fill %s returned other outputs" % (what, f)
        for n, t in ref.items():
            o = out[n]
            assert o.shape == t.shape and o.dtype == t.dtype, "%s: %s under fill %s: shape / dtype" % (what, n, f)
            if not torch.equal(o, t):
                bad = (o != t) | (o != o) if t.dtype.is_floating_point else (o != t)
                raise AssertionError("%s: %s depends on the scratch memory: fill %s differs from fill Z in %d of %d elements"
                                     % (what, n, f, int(bad.sum()), t.numel()))
