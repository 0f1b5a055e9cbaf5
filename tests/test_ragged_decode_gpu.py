"""Ragged batched decode on the GPU: per-sequence positions in the
decode kernels, the models over a slot pool, and the graph-captured
scheduler step."""

import pytest
import torch

import ragged_cases as rc
from mlx_sharding_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


def ext():
    from mlx_sharding_amd import ops
    e = ops.hip_ext()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _close(a, b, atol, rtol=1e-2):
    a = a.float().cpu()
    b = b.float().cpu()
    err = (a - b).abs().max().item()
    scale = b.abs().max().item()
    assert err <= atol + rtol * scale, f"max err {err} (scale {scale})"


def _pos(values):
    return torch.tensor(values, dtype=torch.int32, device="cuda")


# -- 1. attn_decode with pos=[B] ----------------------------------------------

SCAP = 1024


@pytest.mark.parametrize("Hq,Hkv,Dk,Dv,lengths,softcap,window,alias", [
    (8, 2, 128, 128, (1, 257, 700), 0.0, 0, False),
    (16, 1, 576, 512, (1, 257, 700), 0.0, 0, True),   # absorbed MLA
    (8, 4, 128, 128, (5, 300, 700), 50.0, 256, False),
])
def test_attn_decode_per_row_positions(Hq, Hkv, Dk, Dv, lengths, softcap,
                                       window, alias):
    torch.manual_seed(0)
    B = len(lengths)
    scale = Dk ** -0.5
    q = torch.randn(B, Hq, 1, Dk, dtype=torch.bfloat16, device="cuda")
    kbuf = torch.randn(B, Hkv, SCAP, Dk, dtype=torch.bfloat16, device="cuda")
    if alias:
        vbuf = kbuf[..., :Dv]
    else:
        vbuf = torch.randn(B, Hkv, SCAP, Dv, dtype=torch.bfloat16,
                           device="cuda")
    # rows past each sequence's own length must never be loaded
    for b, n in enumerate(lengths):
        kbuf[b, :, n:] = float("nan")
        if not alias:
            vbuf[b, :, n:] = float("nan")
    out = ext().attn_decode(q, kbuf, vbuf, scale, softcap, window,
                            pos=_pos([n - 1 for n in lengths]))
    assert torch.isfinite(out.float()).all()
    for b, n in enumerate(lengths):
        want = ref.attention(
            q[b:b + 1].cpu(), kbuf[b:b + 1, :, :n].cpu(),
            vbuf[b:b + 1, :, :n].cpu().contiguous(), scale,
            causal_offset=n - 1, softcap=softcap, sliding_window=window)
        _close(out[b:b + 1], want, atol=3e-2)


def test_attn_decode_shared_position_and_host_length_unchanged():
    torch.manual_seed(1)
    B, Hq, Hkv, D, S = 3, 8, 2, 128, 300
    q = torch.randn(B, Hq, 1, D, dtype=torch.bfloat16, device="cuda")
    kbuf = torch.randn(B, Hkv, SCAP, D, dtype=torch.bfloat16, device="cuda")
    vbuf = torch.randn(B, Hkv, SCAP, D, dtype=torch.bfloat16, device="cuda")
    want = ref.attention(q.cpu(), kbuf[:, :, :S].cpu(), vbuf[:, :, :S].cpu(),
                         D ** -0.5, causal_offset=S - 1)
    host = ext().attn_decode(q, kbuf[:, :, :S], vbuf[:, :, :S], D ** -0.5,
                             0.0, 0)
    shared = ext().attn_decode(q, kbuf, vbuf, D ** -0.5, 0.0, 0,
                               pos=_pos([S - 1]))
    _close(host, want, atol=3e-2)
    _close(shared, want, atol=3e-2)
    with pytest.raises(RuntimeError):
        ext().attn_decode(q, kbuf, vbuf, D ** -0.5, 0.0, 0, pos=_pos([1, 2]))


# -- 2. appends with pos=[B] --------------------------------------------------

APPEND_POS = (0, 5, 1023)
SENTINEL = 7.0


def _tables(positions, D):
    """Per-sequence cos/sin [B, 1, D/2] for one new token per row."""
    cos, sin = ref.rope_cos_sin(torch.tensor(positions), ref.rope_freqs(D))
    return cos[:, None, :].contiguous(), sin[:, None, :].contiguous()


@pytest.mark.parametrize("interleaved", [False, True])
def test_rope_append_kv_per_row_positions(interleaved):
    torch.manual_seed(2)
    B, Hkv, D = len(APPEND_POS), 2, 128
    k = torch.randn(B, 1, Hkv, D, dtype=torch.bfloat16, device="cuda")
    v = torch.randn(B, 1, Hkv, D, dtype=torch.bfloat16, device="cuda")
    cos, sin = _tables(APPEND_POS, D)
    kc = torch.full((B, Hkv, SCAP, D), SENTINEL, dtype=torch.bfloat16,
                    device="cuda")
    vc = kc.clone()
    ext().rope_append_kv(k, v, cos.cuda(), sin.cuda(), kc, vc,
                         pos=_pos(APPEND_POS), interleaved=interleaved)
    roped = ref.apply_rope(k.cpu(), cos, sin, interleaved)  # [B,1,Hkv,D]
    want_v = torch.full_like(vc, SENTINEL).cpu()
    untouched = torch.ones(B, Hkv, SCAP, dtype=torch.bool)
    for b, p in enumerate(APPEND_POS):
        want_v[b, :, p] = v[b, 0].cpu()
        untouched[b, :, p] = False
        _close(kc[b, :, p], roped[b, 0], atol=2e-2)
    assert torch.equal(vc.cpu(), want_v)
    assert (kc.cpu()[untouched] == SENTINEL).all(), "K written elsewhere"


@pytest.mark.parametrize("nh,nope,vd,rope", [
    (4, 32, 32, 16),    # expanded layout
    (1, 64, 0, 16),     # compressed rows [c_kv | k_pe], no V
])
def test_mla_append_kv_per_row_positions(nh, nope, vd, rope):
    torch.manual_seed(3)
    B = len(APPEND_POS)
    kvh = torch.randn(B, 1, nh, nope + vd, dtype=torch.bfloat16,
                      device="cuda")
    kpe = torch.randn(B, 1, rope, dtype=torch.bfloat16, device="cuda")
    kc = torch.full((B, nh, SCAP, nope + rope), SENTINEL,
                    dtype=torch.bfloat16, device="cuda")
    vc = torch.full((B, nh, SCAP, vd), SENTINEL, dtype=torch.bfloat16,
                    device="cuda")
    want_k, want_v = kc.clone(), vc.clone()
    for b, p in enumerate(APPEND_POS):
        want_k[b, :, p, :nope] = kvh[b, 0, :, :nope]
        want_k[b, :, p, nope:] = kpe[b, 0]
        want_v[b, :, p] = kvh[b, 0, :, nope:]
    ext().mla_append_kv(kvh, kpe, kc, vc, pos=_pos(APPEND_POS))
    assert torch.equal(kc, want_k)
    assert torch.equal(vc, want_v)


# -- 3. apply_rope with [B, T, D/2] tables ------------------------------------

@pytest.mark.parametrize("interleaved", [False, True])
def test_apply_rope_per_sequence_tables(interleaved):
    torch.manual_seed(4)
    B, T, nH, Hkv, D = 3, 5, 4, 2, 64
    starts = (0, 9, 130)
    inv = ref.rope_freqs(D)
    tabs = [ref.rope_cos_sin(torch.arange(s, s + T), inv) for s in starts]
    cos = torch.stack([c for c, _ in tabs])   # [B, T, D/2]
    sin = torch.stack([s for _, s in tabs])
    x = torch.randn(B, T, nH, D, dtype=torch.bfloat16, device="cuda")
    y = ext().apply_rope(x, cos.cuda(), sin.cuda(), interleaved)
    _close(y, ref.apply_rope(x.cpu(), cos, sin, interleaved), atol=2e-2)
    # strided q view of a fused-QKV output, read in place
    qkv = torch.randn(B, T, (nH + 2 * Hkv) * D, dtype=torch.bfloat16,
                      device="cuda")
    qv = qkv[..., : nH * D].view(B, T, nH, D)
    assert not qv.is_contiguous()
    y = ext().apply_rope(qv, cos.cuda(), sin.cuda(), interleaved)
    _close(y, ref.apply_rope(qv.cpu(), cos, sin, interleaved), atol=2e-2)


# -- 4. model level -----------------------------------------------------------

@pytest.mark.parametrize("name", ["llama", "debug-deepseek"])
def test_ragged_decode_gpu_matches_cpu_solo(name):
    model = rc.build_model(name)
    prompts, forced = rc.sequences(model.config.vocab_size)
    want = [rc.solo_run(model, p, f) for p, f in zip(prompts, forced)]
    got = rc.ragged_run(model.to("cuda"), prompts, forced)
    for i in range(len(prompts)):
        for step, (a, b) in enumerate(zip(got[i], want[i])):
            assert torch.isfinite(a).all(), f"{name} seq {i} step {step}"
            _close(a, b, atol=6e-2)


# -- 5. graph -------------------------------------------------------------------

def test_scheduler_graph_replay_matches_eager(monkeypatch):
    from mlx_sharding_amd.parallel.batching import BatchScheduler
    from mlx_sharding_amd.parallel.engine import SamplingParams

    prompts, _ = rc.sequences(128)

    def run(graph: bool):
        monkeypatch.setenv("MLXS_AMD_SERVE_GRAPH", "1" if graph else "0")
        model = rc.build_model("llama", "cuda")
        # "cuda" without an index is what the API server passes
        sched = BatchScheduler(model, max_batch=4, capacity=64, device="cuda")
        try:
            first = sched.submit(prompts[0], SamplingParams(max_tokens=12))
            # two tokens out: the step has already run when the next
            # requests are admitted, so their eager prefills land
            # between two replays of the captured step
            out = [[next(first)[0], next(first)[0]], [], []]
            assert sched.graphed == graph
            second = sched.submit(prompts[1], SamplingParams(max_tokens=9))
            out[1].append(next(second)[0])
            third = sched.submit(prompts[2], SamplingParams(max_tokens=7))
            for i, s in enumerate((first, second, third)):
                out[i] += [t for t, _ in s]
            return out
        finally:
            sched.close()

    eager = run(False)
    captured = run(True)
    assert [len(o) for o in eager] == [12, 9, 7]
    assert eager == captured, f"{eager} vs {captured}"
