"""The sample_rows HIP kernel against the fp64 specification on every case
of sample_cases.py (exact ids, bit-equal edits, untouched inactive rows),
its determinism, graph capture, the [B, 1] ids view and the binding's
limits."""

import numpy as np
import pytest
import torch

import sample_cases as sc
from mlx_sharding_amd import ops

pytestmark = pytest.mark.gpu

ALL = sc.cases() + sc.dyadic_cases()
IDS = [c["name"] for c in ALL]
LSE_ATOL = 2e-4   # the worst-order fp32 sum error (sample_cases.py)


def ext():
    e = ops.hip_ext()
    assert e is not None, "HIP extension must be built on a GPU box"
    return e


def _launch(a):
    ext().sample_rows(a["logits"], a["temperature"], a["top_p"], a["u"],
                      a["active"], a["ids_out"], a["lse_out"], a["bias_idx"],
                      a["bias_val"], a["pen_idx"], a["penalty"])


@pytest.mark.parametrize("case", ALL, ids=IDS)
def test_kernel_equals_fp64_spec(case):
    a = sc.torch_args(case, "cuda")
    _launch(a)
    ids = a["ids_out"].cpu().numpy()
    lse = a["lse_out"].cpu().numpy()
    logits = a["logits"].cpu().numpy()
    on = case["active"] != 0
    print(case["name"], "max |lse - fp64| =",
          np.abs(lse - case["want_lse"])[on].max())
    assert ids.tolist() == case["want_ids"].tolist()
    # edits bit-equal to the reference's; inactive rows as they were
    ref_args = sc.torch_args(case)
    ops.sample_rows(**ref_args)
    assert np.array_equal(logits, ref_args["logits"].numpy())
    assert np.array_equal(logits[~on], case["logits"][~on])
    assert np.array_equal(ids[~on], case["ids_init"][~on])
    assert np.array_equal(lse[~on], case["lse_init"][~on])
    assert np.abs(lse - case["want_lse"])[on].max() <= LSE_ATOL


def test_two_launches_give_identical_ids():
    for case in (sc.cases()[-1], sc.cases()[6]):
        runs = []
        for _ in range(2):
            a = sc.torch_args(case, "cuda")
            _launch(a)
            runs.append((a["ids_out"].cpu(), a["lse_out"].cpu()))
        assert torch.equal(runs[0][0], runs[1][0])
        assert torch.equal(runs[0][1], runs[1][1])


def test_ids_out_as_a_column_view():
    case = sc.cases()[5]
    a = sc.torch_args(case, "cuda")
    tok = a["ids_out"].clone().view(-1, 1)
    a["ids_out"] = tok
    _launch(a)
    assert tok.view(-1).tolist() == case["want_ids"].tolist()


def test_graph_replay_follows_new_inputs():
    first = sc.cases()[5]   # V = 1000
    a = sc.torch_args(first, "cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _launch(sc.torch_args(first, "cuda"))      # warm-up
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _launch(a)
    # same buffers, new contents: the case with its rows rolled by one,
    # so every row sees other logits, parameters and another u
    B = a["logits"].shape[0]
    perm = [(b + 1) % B for b in range(B)]
    rolled = {k: v[perm].copy() if isinstance(v, np.ndarray) else v
              for k, v in first.items()}
    fresh = sc.torch_args(rolled, "cuda")
    for k, t in a.items():
        if t is not None:
            t.copy_(fresh[k])
    g.replay()
    torch.cuda.synchronize()
    assert a["ids_out"].cpu().tolist() == rolled["want_ids"].tolist()
    assert rolled["want_ids"].tolist() != first["want_ids"].tolist()


def _args(B=2, V=16, NB=2, W=3):
    dev = "cuda"
    return dict(
        logits=torch.zeros(B, V, device=dev),
        temperature=torch.ones(B, device=dev),
        top_p=torch.ones(B, device=dev), u=torch.zeros(B, device=dev),
        active=torch.ones(B, dtype=torch.int32, device=dev),
        ids_out=torch.zeros(B, dtype=torch.int64, device=dev),
        lse_out=torch.zeros(B, device=dev),
        bias_idx=torch.full((B, NB), -1, dtype=torch.int32, device=dev),
        bias_val=torch.zeros(B, NB, device=dev),
        pen_idx=torch.full((B, W), -1, dtype=torch.int32, device=dev),
        penalty=torch.ones(B, device=dev))


def _raises(match, **change):
    a = _args()
    a.update(change)
    with pytest.raises(RuntimeError, match=match):
        _launch(a)


def test_binding_limits_raise():
    _launch(_args())   # the unchanged arguments pass
    dev = "cuda"
    _raises("logits", logits=torch.zeros(2, 16, device=dev).half())
    _raises("logits", logits=torch.zeros(2, 32, device=dev)[:, ::2])
    _raises("logits", logits=torch.zeros(2, 4, 4, device=dev))
    for name in ("temperature", "top_p", "u", "lse_out", "penalty"):
        _raises(name, **{name: torch.ones(3, device=dev)})
        _raises(name, **{name: torch.ones(2, device=dev).double()})
    _raises("active", active=torch.ones(2, dtype=torch.int64, device=dev))
    _raises("active", active=torch.ones(1, dtype=torch.int32, device=dev))
    _raises("ids_out", ids_out=torch.zeros(2, dtype=torch.int32, device=dev))
    _raises("ids_out", ids_out=torch.zeros(3, dtype=torch.int64, device=dev))
    _raises("ids_out",
            ids_out=torch.zeros(2, 2, dtype=torch.int64, device=dev))
    _raises("bias_idx", bias_idx=torch.full((2, 33), -1, dtype=torch.int32,
                                            device=dev),
            bias_val=torch.zeros(2, 33, device=dev))
    _raises("bias_idx", bias_idx=torch.full((2, 2), -1, device=dev).long())
    _raises("bias_val", bias_val=torch.zeros(2, 2, device=dev).double())
    _raises("same shape", bias_val=torch.zeros(2, 3, device=dev))
    _raises("pen_idx", pen_idx=torch.full((2, 65), -1, dtype=torch.int32,
                                          device=dev))
    _raises("pen_idx", pen_idx=torch.full((3, 3), -1, dtype=torch.int32,
                                          device=dev))
    _raises("together", bias_val=None)
    _raises("together", bias_idx=None)
    _raises("together", penalty=None)
    _raises("together", pen_idx=None)
    # at the limits
    _launch(_args(NB=32, W=64))
    torch.cuda.synchronize()
