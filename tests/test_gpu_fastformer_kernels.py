"""Per-kernel tests (-m gpu) of csrc/fastformer.hip: launch_ff_pool (ff_pool_partial_kernel in its five instantiations + ff_pool_merge_kernel)
and launch_ff_scale, one launch at a time through tests/csrc/fastformer_harness.hip (tests/fastformer_harness.py), at the cases of
tests/fastformer_kernel_cases.py against the restatements of tests/fastformer_kernel_ref.py.

Every launch runs on guarded buffers (tests/test_gpu_kernels.py's Guarded): NaN bands around every buffer, NaN in the row gaps of a strided v,
`out` and the workspace pre-filled with a sentinel, the workspace of exactly the bytes the library reports; bands and gaps must hold their
bits afterwards and the inputs must be unchanged.

Exact tier (bit for bit): uniform weights, two-level logits, the workspace's run maxima against the restated logits (every case, Gaussian
data included), single-row runs, RP = 4 against RP = 2 on the same rows, repeat-call stability, ff_scale.  General tier: Gaussian data under
the bar derived in fastformer_kernel_ref.py and the aggregate rule.  Every case asserts which instantiation it takes from the restated
ff_shape, tied to the library's ff_pool_splits / ff_pool_workspace_bytes."""
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import fastformer_kernel_cases as fc   # noqa: E402
import fastformer_kernel_ref as fr     # noqa: E402
from test_gpu_kernels import BAND, Guarded, i32, record   # noqa: E402

pytestmark = pytest.mark.gpu

f32 = np.float32
SENT = f32(-12345.5)
_T0 = time.time()
_tally = {}
_seen = set()


@pytest.fixture(scope="module")
def fh():
    import torch
    assert torch.cuda.is_available(), "the kernel tests need the GPU"
    import fastformer_harness
    import __graft_entry__ as g
    assert g.built_harness_fastformer_hash() == g.harness_fastformer_hash(), "libe2etts_kernels_test.so was not built from this tree: run build()"
    fastformer_harness.load()
    assert g.harness_fastformer_hash() in fastformer_harness.version()
    return fastformer_harness


def tally(family, **fig):
    t = _tally.setdefault(family, dict(launches=0, elements=0, differing=0, worst=0.0, agg=0.0))
    t["launches"] += 1
    t["elements"] += fig.get("elements", 0) + fig.get("maxima", 0)
    t["differing"] += fig.get("differing", 0) + fig.get("maxima_differing", 0)
    t["worst"] = max(t["worst"], fig.get("worst") or 0.0)
    t["agg"] = max(t["agg"], fig.get("agg") or 0.0)


class Launch:
    """The device buffers of one launch_ff_pool call and the call itself."""

    def __init__(self, fh, d, B, N, H, hs, pad=0):
        self.fh, self.dims = fh, (B, N, H, hs)
        self.v = Guarded(d["v"], ld=H + pad)
        self.scale = Guarded(d["scale"]) if d["scale"] is not None else None
        self.wl, self.bl = Guarded(d["wl_t"]), Guarded(d["bl"])
        self.lens = i32(d["lens"]) if d["lens"] is not None else None
        self.ws_bytes, self.splits = fh.workspace_bytes(B, N, H, hs), fh.splits(B, N, H, hs)
        assert self.ws_bytes == B * self.splits * (H // hs) * (hs + 2) * 4 > 0
        self.ws = Guarded(shape=(self.ws_bytes // 4,), sentinel=SENT)       # exactly the bytes reported; a NaN band follows
        self.out = Guarded(shape=(B, H), sentinel=SENT)

    def run(self):
        B, N, H, hs = self.dims
        msg = self.fh.ff_pool(self.v.ptr, self.v.ld, self.scale.ptr if self.scale else None, self.wl.ptr, self.bl.ptr,
                              self.lens.data_ptr() if self.lens is not None else None, self.out.ptr, self.ws.ptr, self.ws_bytes, B, N, H, hs)
        assert msg is None, msg
        out, ok_o = self.out.fetch()
        ws, ok_w = self.ws.fetch()
        assert ok_o and ok_w, "a guard band of out or of the workspace was written"
        for g in (self.v, self.scale, self.wl, self.bl):
            assert g is None or g.unchanged(), "an input buffer, its row gaps or its guard band was written"
        return out.reshape(B, H).copy(), ws.reshape(B, self.splits, H // hs, hs + 2).copy()

    def poison_workspace(self):
        self.ws.dev[BAND:BAND + self.ws_bytes // 4] = float("nan")


def launch_case(fh, name):
    c, ref = fc.ALL[name], fc.reference(name)
    L = Launch(fh, fc.inputs(name), c["B"], c["N"], c["H"], c["hs"], c["pad"])
    fails = fc.check_shape(ref, L.splits, L.ws_bytes)
    assert not fails, fails
    _seen.add((ref["sh"]["rp"], ref["sh"]["maxt"]))
    out, ws = L.run()
    assert not np.any(out == SENT) and not np.any(ws == SENT), "an element of out or of the workspace was not written"
    return c, ref, L, out, ws


# ---------------------------------------------------------------- general tier (+ the logit check on its workspaces)
@pytest.mark.parametrize("name", [c["name"] for c in fc.GENERAL])
def test_pool_general(fh, name):
    c, ref, L, out, ws = launch_case(fh, name)
    fails, fig = fc.check_general(ref, out)
    print(f"[fastformer kernels] {name}: worst error / bar {fig['worst']:.3g}, aggregate ratio {fig['agg']}")
    tally("ff_pool general", **fig)
    wfails, wfig = fc.check_workspace(ref, ws)
    tally("ff_pool run maxima (Gaussian)", **wfig)
    assert not fails and not wfails, fails + wfails


@pytest.mark.parametrize("name", ["rp4_h8_hs1_n33_scale", "rp2_1024_h512_hs1_n33", "rp1_h768_hs2_n17", "multi_tile_n16385"])
def test_pool_repeat_call_is_bit_identical(fh, name):
    """A second call on a workspace poisoned in between: no entry of the workspace is read before it is written, nothing depends on the run."""
    c, ref, L, out, ws = launch_case(fh, name)
    L.poison_workspace()
    out2, ws2 = L.run()
    nd = fr.diff_count(out, out2) + fr.diff_count(ws, ws2)
    tally("ff_pool repeat call", elements=out.size + ws.size, differing=nd)
    assert nd == 0


# ---------------------------------------------------------------- exact tier
@pytest.mark.parametrize("name", [c["name"] for c in fc.UNIFORM + fc.TWO_LEVEL])
def test_pool_exact(fh, name):
    """Uniform weights (wl = 0, a bias) and two-level logits on dyadic values: out is the mean of the selected rows, one rounding."""
    c, ref, L, out, ws = launch_case(fh, name)
    fails, fig = fc.check_exact(ref, out)
    tally(f"ff_pool exact ({c['kind']})", **fig)
    wfails, wfig = fc.check_workspace(ref, ws)
    tally("ff_pool run maxima (exact tier)", **wfig)
    assert not fails and not wfails, fails + wfails


def test_pool_rp4_equals_rp2(fh):
    """The same 600 rows alone (RP = 4) and as one row of a batch of 14 (RP = 2), 16 rows per run both times: out and the workspace rows
    bit-identical ("same bits for every RP")."""
    N, H, hs, B, row = fc.RP_N, fc.RP_H, fc.RP_HS, fc.RP_B, fc.RP_ROW
    one, many = fr.ff_shape(1, N, H, hs), fr.ff_shape(B, N, H, hs)
    assert (one["rp"], many["rp"]) == (4, 2) and one["rows_per_wg"] == many["rows_per_wg"] == 16 and one["splits"] == many["splits"]
    r = fc.rng_of("ffk_rp4_rp2")
    v = r.standard_normal((B, N, H)).astype(f32)
    d = dict(v=v, scale=r.standard_normal((B, H)).astype(f32), wl_t=(r.standard_normal((H, H // hs)) / 8).astype(f32),
             bl=r.standard_normal(H // hs).astype(f32), lens=[N - 7 * b for b in range(B)])
    d1 = dict(d, v=v[row:row + 1], scale=d["scale"][row:row + 1], lens=d["lens"][row:row + 1])
    La, Lb = Launch(fh, d, B, N, H, hs, pad=4), Launch(fh, d1, 1, N, H, hs)
    assert (La.splits, Lb.splits) == (many["splits"], one["splits"])
    _seen.update({(4, 512), (2, 512)})
    (oa, wa), (ob, wb) = La.run(), Lb.run()
    nd = fr.diff_count(oa[row:row + 1], ob) + fr.diff_count(wa[row:row + 1], wb)
    tally("ff_pool RP 4 = RP 2", elements=ob.size + wb.size, differing=nd)
    assert nd == 0
    s = fr.logits_f32(d1["v"], d1["scale"], d["wl_t"], d["bl"], d1["lens"], hs)            # and both are the restated logits
    assert fr.diff_count(wb[..., 0], fr.run_maxima(s, N, one)) == 0


@pytest.mark.parametrize("name", [c[0] for c in fc.SCALE_CASES])
def test_scale(fh, name):
    """ff_scale: both outputs bit for bit; q_ld = H and 2 H, totals on and off 1024 elements, H = 4, signed zeros, subnormals, infinities."""
    _, B, N, H, q_ld = next(c for c in fc.SCALE_CASES if c[0] == name)
    q, gk, x = fc.scale_inputs(name)
    gq, gg, gx = Guarded(q, ld=q_ld), Guarded(gk), Guarded(x)
    gw, go = Guarded(shape=(B, N, H), sentinel=SENT), Guarded(shape=(B, N, H), sentinel=SENT)
    assert fh.ff_scale(gq.ptr, q_ld, gg.ptr, gx.ptr, gw.ptr, go.ptr, B, N, H) is None
    (wv, ok1), (qx, ok2) = gw.fetch(), go.fetch()
    assert ok1 and ok2 and gq.unchanged() and gg.unchanged() and gx.unchanged()
    fails, fig = fc.check_scale(name, wv, qx)
    tally("ff_scale", **fig)
    assert not fails, fails


def test_every_instantiation_ran_and_tally():
    """All five instantiations of ff_pool_partial_kernel were executed by a case that asserted which one it got; launches judged, elements
    compared and the worst ratios: printed and recorded."""
    assert _seen == {(4, 512), (4, 1024), (2, 512), (2, 1024), (1, 512)}, _seen
    for fam, t in sorted(_tally.items()):
        print(f"[fastformer kernels] {fam}: {t['launches']} launches, {t['elements']} elements, {t['differing']} differing, worst error / bar {t['worst']:.3g}, "
              f"worst aggregate ratio {t['agg']:.3g}")
        record("fastformer_kernels", kernel=fam, **t)
    record("fastformer_kernels_wall", seconds=time.time() - _T0)
    print(f"[fastformer kernels] wall time {time.time() - _T0:.1f} s")
