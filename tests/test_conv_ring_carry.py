"""The staggered conv kernel's weight ring across part, tap and unit boundaries (vge_encoder_x3s.hip), and the
conv-done event of the same launch path (vge_encoder_wait_conv).

The ring is primed before the barrier in front of a GEMM's part 0 and carried from part 0 into part 1, so what can go
wrong sits where a part, a tap or a unit meets it: a chunk in the wrong slot, the wrong next part, a missing window.
The batch sizes walk the unit kinds of the schedule: 1 = a pair with a missing window, 2 = a full pair, 4 = one quad,
5 = a quad + a short pair, 6 = a quad + a pair, 37 = several rounds with a partial last one.

Tolerances are the existing ones: f32x3 against the exact-f32 path on the same input 2e-5 on the embeddings and 1e-5 on
the window TC (tests/test_gpu_parity.py, test_x3_quad_and_pair_blocks_vs_f32); f16 2e-4 on the embeddings and 1e-4 on
TC (tests/test_bench_parity.py); two equally valid f32 summation orders 2e-6 (tests/test_bench_parity.py,
tests/test_encoder_shapes.py).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BATCHES = [1, 2, 4, 5, 6, 37]
TOL = {"f32x3": (2e-5, 2e-5, 1e-5), "f16": (2e-4, 2e-4, 1e-4)}  # seq, frame embeddings, window TC
F32_ORDER = 2e-6


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vge import ops
    return ops


@pytest.fixture(scope="module")
def sd():
    from vge import synth
    return synth.make_state_dict(synth.DIMS_RAW, synth.DIMS_DIFF)


@pytest.fixture(scope="module")
def feats(ops):
    g = torch.Generator().manual_seed(20)
    return torch.randn(37, 32, 2596, generator=g).to(DEV)


@pytest.fixture(scope="module")
def exact(ops, sd, feats):
    """The exact-f32 path on the first B windows, once per batch size."""
    enc = ops.Encoder(sd, device=DEV, compute="f32")
    out = {B: enc.encode(feats[:B].contiguous(), frame_embed=True, tc=True) for B in BATCHES}
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module", params=["f32x3", "f16"])
def staggered(ops, sd, request):
    return request.param, ops.Encoder(sd, device=DEV, compute=request.param)


@pytest.mark.parametrize("B", BATCHES)
def test_unit_kinds_vs_exact_f32(staggered, feats, exact, B):
    compute, enc = staggered
    got = enc.encode(feats[:B].contiguous(), frame_embed=True, tc=True)
    err = [(a - b).abs().max().item() for a, b in zip(got, exact[B])]
    print(f"{compute} B={B}: seq {err[0]:.2e} frame {err[1]:.2e} tc {err[2]:.2e}")
    for e, tol in zip(err, TOL[compute]):
        assert e < tol, (err, TOL[compute])
    enc.status()


def test_window_gives_the_same_result_in_a_quad_row_and_in_a_pair_row(staggered, feats):
    """One window at position 0 of a batch of 4 (a quad's row) and at position 4 of a batch of 6 (a pair's row)."""
    compute, enc = staggered
    w = feats[7:8]
    in_quad = torch.cat([w, feats[10:13]]).contiguous()
    in_pair = torch.cat([feats[20:24], w, feats[30:31]]).contiguous()
    q = enc.encode(in_quad, frame_embed=True, tc=True)
    q2 = enc.encode(in_quad, frame_embed=True, tc=True)
    p = enc.encode(in_pair, frame_embed=True, tc=True)
    p2 = enc.encode(in_pair, frame_embed=True, tc=True)
    torch.cuda.synchronize()
    for a, b in list(zip(q, q2)) + list(zip(p, p2)):
        assert torch.equal(a, b)
    err = [(a[0] - b[4]).abs().max().item() for a, b in zip(q, p)]
    print(f"{compute}: quad row vs pair row: seq {err[0]:.2e} frame {err[1]:.2e} tc {err[2]:.2e}")
    assert max(err) < F32_ORDER, err


def test_wait_conv_orders_an_overwrite_of_feats_after_the_conv_stage(ops, sd, feats):
    """On a fresh encoder: encode, wait_conv(side), overwrite the feats buffer on `side`, encode again, twice.  The
    conv stage is the last reader of feats, so both encodes must give what they give on an untouched buffer."""
    n = 256  # a conv stage long enough (~1 ms) for an unordered overwrite to land inside it
    g = torch.Generator().manual_seed(21)
    a = torch.randn(n, 32, 2596, generator=g).to(DEV)
    b = torch.randn(n, 32, 2596, generator=g).to(DEV)
    ref = ops.Encoder(sd, device=DEV, compute="f32x3")
    want_a = ref.encode(a, frame_embed=True, tc=True)
    want_b = ref.encode(b, frame_embed=True, tc=True)
    torch.cuda.synchronize()

    enc = ops.Encoder(sd, device=DEV, compute="f32x3")
    enc.reserve(n)
    buf = a.clone()
    side = torch.cuda.Stream(device=DEV)
    main = torch.cuda.current_stream(DEV)
    torch.cuda.synchronize()
    got = []
    for nxt in (b, a):
        got.append(enc.encode(buf, frame_embed=True, tc=True))
        enc.wait_conv(side)
        with torch.cuda.stream(side):
            buf.copy_(nxt)
        main.wait_stream(side)
    torch.cuda.synchronize()
    for x, y in list(zip(got[0], want_a)) + list(zip(got[1], want_b)):
        assert torch.equal(x, y)
    enc.status()
