"""What the patch-dropout tests share (tests/test_patch_drop_cpu.py, tests/test_gpu_patch_drop.py): the (B, N, K)
cases of the keep table, its defining properties, and the oracle composed for a model that runs on a subset of the
tokens — oracle.embed_forward, a gather of the kept tokens (the patches of the table, then CLS), oracle.block_forward
for every block on the [B, K + 1, D] tensor (so the dropout keep bits are drawn at the compacted tensor's indices),
oracle.head_forward.  The oracle itself is called unchanged."""
import torch
import torch.nn.functional as F

from oracle import vit_oracle as O

# (B, N, K): the smallest tables, K = 1 and K = N, more images than threads need, more than 256 patches (several per
# thread), 4096 patches (the cap)
CASES = [(1, 1, 1), (3, 2, 1), (3, 2, 2), (5, 16, 8), (4, 36, 27), (257, 196, 98), (2, 576, 288), (2, 1024, 1),
         (2, 1024, 1024), (2, 4096, 2048)]

BASE_SEED = 195950210         # what torch.manual_seed(42) makes a forward draw


def check_table(idx, inv, B, N, K):
    """The defining properties of a keep table: idx [B, K] ascending and unique with column 0 equal to 0, inv [B, N]
    its inverse (-1 where dropped)."""
    assert idx.dtype == torch.int32 and inv.dtype == torch.int32
    assert tuple(idx.shape) == (B, K) and tuple(inv.shape) == (B, N)
    i64 = idx.long()
    assert bool((i64[:, 0] == 0).all())
    assert bool((i64[:, 1:] > i64[:, :-1]).all())                      # ascending, hence unique
    assert int(i64.min()) >= 0 and int(i64.max()) < N
    want = torch.full((B, N), -1, dtype=torch.int32)
    want.scatter_(1, i64, torch.arange(K, dtype=torch.int32).expand(B, K))
    assert torch.equal(inv, want)


def gather_tokens(e, idx):
    """[B, N + 1, D] -> [B, K + 1, D]: the patches idx [B, K] names, then the CLS token (row N)."""
    B, T, D = e.shape
    rows = torch.cat([idx.long(), torch.full((B, 1), T - 1, dtype=torch.long)], dim=1)
    return e.gather(1, rows[:, :, None].expand(-1, -1, D))


def oracle_run(st, x, y, ocfg, idx, seed=BASE_SEED, masks=None, bf16=False, dtype=torch.float32):
    """(logits, loss, {key: grad}, input-image grad) of a training step on the tokens of `idx`.  `masks`: explicit
    {(l, site): [B, K + 1, D]} masks instead of the element dropout's hash draw under `seed` (drop path: the two
    masks combined, as tests/test_gpu_drop_path.py hands them to the oracle)."""
    rnd = O._RoundBF16.apply if bf16 else O._identity
    params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in st.items()}
    xin = x.detach().to(dtype).clone().requires_grad_(True)
    e = gather_tokens(O.embed_forward(params, xin, ocfg, rnd, bf16), idx)
    for l in range(ocfg.num_blocks):
        e, _ = O.block_forward(params, l, e, ocfg, rnd, train=True, seed=seed, masks=masks)
    logits = O.head_forward(params, e)
    loss = F.cross_entropy(logits, y)
    loss.backward()
    return logits.detach(), loss.detach(), {k: p.grad for k, p in params.items()}, xin.grad


def check_fp32(got, ref, what=""):
    """The fp32 model gates of tests/test_gpu_drop_path.py::test_model_fp32_vs_oracle: logits 1e-4, loss 1e-5, every
    gradient (the input image's too) 2e-4 of max(1, its largest entry).  Prints each figure before asserting."""
    (logits, loss, grads, dimg), (lg_ref, loss_ref, g_ref, dimg_ref) = got, ref
    err = (logits.double() - lg_ref.double()).abs().max().item()
    lerr = abs(float(loss) - float(loss_ref))
    print(f"{what} fp32: logits max err {err:.3e}, loss err {lerr:.3e}")
    rows = []
    for k, g in list(grads.items()) + [("input image", dimg)]:
        r = dimg_ref if k == "input image" else g_ref[k]
        e = (g.double() - r.double()).abs().max().item()
        rows.append((e / max(1.0, r.abs().max().item()), k))
    print(f"{what} fp32: worst gradient errors (of max(1, |g|max)):", sorted(rows)[-3:])
    assert err < 1e-4
    assert lerr < 1e-5
    for e, k in rows:
        assert e == e and e <= 2e-4, (k, e)


def rel(a, b):
    return float((a.double() - b.double()).norm() / max(float(b.double().norm()), 1e-30))


def check_bf16(got, ref_bf, ref_32, what=""):
    """The bf16 model gates of tests/test_gpu_drop_path.py::test_model_bf16_vs_oracle_same_rounding: logits within
    1e-2 (norm-wise) of the oracle with bf16 storage rounding; every gradient's error against the fp32 oracle at most
    max(1e-2, 2 x that bf16 oracle's own error against it)."""
    logits, loss, grads, dimg = got
    e = rel(logits.float(), ref_bf[0])
    print(f"{what} bf16: logits rel err {e:.3e}, loss {float(loss):.5f} (oracle bf16 {float(ref_bf[1]):.5f})")
    rows = []
    for k, g in list(grads.items()) + [("input image", dimg)]:
        r32 = ref_32[3] if k == "input image" else ref_32[2][k]
        rbf = ref_bf[3] if k == "input image" else ref_bf[2][k]
        ours, ora = rel(g.float(), r32), rel(rbf, r32)
        rows.append((ours / max(ora, 1e-9), k, ours, ora))
    print(f"{what} bf16: worst gradient error ratios:", sorted(rows)[-3:])
    assert float(loss) == float(loss) and e < 1e-2
    for _, k, ours, ora in rows:
        assert ours <= max(1e-2, 2 * ora), (k, ours, ora)
