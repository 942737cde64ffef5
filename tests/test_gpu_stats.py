"""The corpus-statistics library on the GPU (libe2etts_stats_test.so) against what the reference's own text computed
(tests/golden/stats_cases.npz) and the numpy restatement (tests/stats_ref.py): the sort, every discrete figure bit for bit, the sums
under the derived bars, every row of a ragged batch against its own B = 1 call, the batching independence of the merge, the refusals
and the data loader's energy target.  The padding of every batch is NaN: nothing beyond a row's length may be read."""
import ctypes as C

import numpy as np
import pytest

import stats_cases as sc
import stats_ref as sr
from e2e_tts_amd import stats as stlib
from test_stats_host import want_stats

pytestmark = pytest.mark.gpu

KIND = {"f0": stlib.F0, "energy": stlib.ENERGY, "pitch": stlib.PITCH}
NAMES = ("lengths", "ragged0", "ragged1", "ragged2", "ties", "outliers", "fences", "constant", "voicing", "twelve")


@pytest.fixture(scope="module")
def st():
    s = stlib.CorpusStats()
    yield s
    s.close()


@pytest.fixture(scope="module")
def gold():
    return sc.load()


@pytest.fixture(scope="module")
def corpora(gold):
    c = sc.corpora()
    for name, utts in c.items():
        assert np.array_equal(sc.digest(utts), gold[f"{name}/digest"])
    return c


def add(st, utts, key):
    x, lens = sc.batch(utts, key)
    st.add(**{key: x}, lens=lens)


def rows_of(st, utts, key):
    add(st, utts, key)
    return st.rows()


def bits(a):
    return np.ascontiguousarray(np.atleast_1d(a)).view(np.uint8).tobytes()


@pytest.mark.parametrize("name", ["lengths", "ties", "ragged2", "constant"])
def test_sorted_rows_equal_np_sort(st, corpora, name):
    x, lens = sc.batch(corpora[name], "energy")
    got = st.sorted_rows(x, lens)
    for b, n in enumerate(lens):
        assert np.array_equal(got[b, :n], np.sort(x[b, :n])), (name, b, n)
        assert np.isnan(got[b, n:]).all()                      # nothing is written beyond a row
    # -0.0 sorts below +0.0, whatever the network: the keys are a total order
    z = np.array([[0.0, -0.0, 1.0, -0.0, 0.0, -1.0, 0.0]], np.float32)
    s = st.sorted_rows(z, [7])[0]
    assert np.array_equal(s, np.sort(z[0])) and list(np.signbit(s)) == [True, True, True, False, False, False, False]


@pytest.mark.parametrize("name", NAMES)
def test_rows_equal_the_reference_bit_for_bit(st, gold, corpora, name):
    """p25, p75, lower, upper, n_kept, min and max exactly; sum, mean and m2 under the bars."""
    st.reset()
    for key in ("energy", "pitch"):
        rows = rows_of(st, corpora[name], key)
        for f in ("p25", "p75", "lower", "upper"):
            assert bits(rows[f]) == bits(gold[f"{name}/{key}/{f}"]), (key, f, rows[f], gold[f"{name}/{key}/{f}"])
        assert np.array_equal(rows["n_kept"], gold[f"{name}/{key}/kept"]) and (rows["status"] == 0).all()
        for b, u in enumerate(corpora[name]):
            want = sr.row_record(u[key], sr.ENERGY)
            assert rows["n"][b] == len(u[key]) and bits(rows["min"][b]) == bits(u[key].min()) and bits(rows["max"][b]) == bits(u[key].max())
            got = {k: float(rows[k][b]) for k in ("sum", "mean", "m2")}
            print(name, key, b, got, {k: want[k] for k in got})
            assert sr.check_row(got, want) == [], (key, b)


@pytest.mark.parametrize("name", ["voicing", "lengths", "ties"])
def test_f0_rows(st, corpora, name):
    st.reset()
    rows = rows_of(st, corpora[name], "f0")
    for b, u in enumerate(corpora[name]):
        want = sr.row_record(u["f0"], sr.F0)
        assert rows["n"][b] == len(u["f0"]) and rows["n_kept"][b] == np.count_nonzero(u["f0"]) == want["n_kept"] and rows["status"][b] == 0
        assert sr.check_row({k: float(rows[k][b]) for k in ("sum", "mean", "m2")}, want) == [], b


@pytest.mark.parametrize("name", ["ragged0", "ragged1", "ragged2"])
def test_every_row_of_a_ragged_batch_equals_its_own_call(st, corpora, name):
    """The row's record, all 72 bytes.  The batch's rows start at odd offsets (T is odd in two of the batches) and sit in a workgroup sized for
    the longest row; the single rows are aligned and sit in a workgroup of their own plan."""
    st.reset()
    for key in ("energy", "f0"):
        batch = rows_of(st, corpora[name], key)
        for b, u in enumerate(corpora[name]):
            one = rows_of(st, [u], key)
            assert bits(one[0]) == bits(batch[b]), (key, b, one[0], batch[b])


def test_the_three_batchings_give_identical_bits(st, gold, corpora):
    utts = corpora["twelve"]
    got = []
    for split in ((12,), (5, 7), (1,) * 12):
        st.reset()
        for key in ("energy", "pitch", "f0"):
            i = 0
            for k in split:
                add(st, utts[i:i + k], key)
                i += k
        got.append(st.blocks())
    assert bits(got[0]) == bits(got[1]) == bits(got[2])
    # and that result is the restatement's fold, bit for bit: the same Chan updates in the same order on records within the bars
    ref = sr.corpus(utts)
    b = got[0]
    for key in ("energy", "pitch", "f0"):
        assert b["n_kept"][KIND[key]] == ref[key]["n_kept"] and b["rows"][KIND[key]] == 12 and b["n_frames"][KIND[key]] == sum(len(u[key]) for u in utts)


@pytest.mark.parametrize("name", NAMES)
def test_build_stats_dict_within_the_bars(st, gold, corpora, name):
    st.reset()
    utts = corpora[name]
    for key in ("energy", "pitch", "f0"):
        add(st, utts, key)
    got, want, ref = st.result(), want_stats(gold, name), sr.corpus(utts)
    blocks = st.blocks()
    assert set(got) == {"f0", "energy", "pitch"} and all(isinstance(v, float) for blk in got.values() for v in blk.values())
    for key in ("f0", "energy", "pitch"):
        bad = sr.check_block(got[key], want[key], ref["_bars"][key], key != "f0")
        print(name, key, got[key], want[key])
        assert bad == [], (key, bad)
    for key in ("energy", "pitch"):
        k = KIND[key]
        assert blocks["n_kept"][k] == int(gold[f"{name}/{key}/kept"].sum())
        assert blocks["raw_min"][k] == min(float(u[key].min()) for u in utts) and blocks["raw_max"][k] == max(float(u[key].max()) for u in utts)
    if name == "constant":
        assert got["energy"]["std"] == 1.0 and got["energy"]["mean"] == 5.0 and got["pitch"]["std"] == 1.0


def test_a_poisoned_workspace_changes_nothing(st, corpora):
    utts = corpora["ragged1"]
    st.reset()
    add(st, utts, "energy")
    rows, blocks = st.rows(), st.blocks()
    st.poison_workspace()
    add(st, utts, "energy")
    assert bits(st.rows()) == bits(rows) and bits(st.blocks()) == bits(blocks)
    st.poison_workspace()
    assert st.result() == {}                                   # the poison resets the accumulators


def test_strided_rows_and_device_lengths(st, corpora):
    """A torch view with a row stride is read where it lies; lens may lie on the device (the raw entry point)."""
    import torch
    utts = corpora["ragged0"]
    x, lens = sc.batch(utts, "energy")
    st.reset()
    add(st, utts, "energy")
    want_rows, want = st.rows(), st.blocks()
    wide = torch.full((x.shape[0], x.shape[1] + 37), float("nan"), device="cuda")
    wide[:, :x.shape[1]] = torch.from_numpy(x).cuda()
    view = wide[:, :x.shape[1]]
    assert not view.is_contiguous()
    st.reset()
    st.add(energy=view, lens=lens)
    assert bits(st.rows()) == bits(want_rows) and bits(st.blocks()) == bits(want)
    st.reset()
    dl = torch.from_numpy(lens).cuda()
    st._call("add", stlib.ENERGY, view.data_ptr(), int(view.stride(0)), C.c_void_p(dl.data_ptr()), x.shape[0], x.shape[1])
    assert bits(st.blocks()) == bits(want)


def test_refusals_name_the_row_and_leave_the_handle_usable(st, corpora):
    utts = corpora["ragged1"]
    x, lens = sc.batch(utts, "energy")
    good = None
    for bad_value, row in ((np.nan, 3), (np.inf, 0), (-np.inf, 6)):
        st.reset()
        add(st, utts[:2], "energy")
        good = st.blocks()
        y = x.copy()
        y[row, int(lens[row]) - 1] = bad_value                # inside the row's length
        st.add(energy=y, lens=lens)
        with pytest.raises(ValueError, match=f"row {row} "):
            st.rows()
        with pytest.raises(ValueError, match=f"energy: row {row} of add 1"):
            st.result()
        st.add(energy=x, lens=lens)                            # nothing more is taken until the reset
        with pytest.raises(ValueError, match=f"energy: row {row} of add 1"):
            st.result()
    st.reset()
    add(st, utts[:2], "energy")
    assert bits(st.blocks()) == bits(good)
    f = corpora["voicing"][2]["f0"].copy()
    f[1] = np.nan
    st.add(f0=f[None], lens=[len(f)])
    with pytest.raises(ValueError, match="f0: row 0 of add 1"):
        st.result()
    # a row above the cap is refused before anything is enqueued, by name; the handle's state is untouched
    st.reset()
    add(st, utts[:2], "energy")
    import torch
    long = torch.zeros((2, sc.CAP + 1), device="cuda")
    with pytest.raises(ValueError, match=r"E2EST_MAX_ROW.*row 1"):
        st.add(energy=long, lens=[sc.CAP, sc.CAP + 1])
    assert bits(st.blocks()) == bits(good)
    # accumulators without a kept value
    st.reset()
    st.add(f0=np.zeros((2, 9), np.float32), lens=[9, 4])
    with pytest.raises(RuntimeError, match="f0: no voiced frame"):
        st.result()
    st.reset()
    st.add(energy=np.full((2, 9), 3.0, np.float32), lens=[9, 1])
    with pytest.raises(RuntimeError, match="energy: no value lies inside"):
        st.result()
    st.reset()
    add(st, utts[:2], "energy")
    assert bits(st.blocks()) == bits(good) and set(st.result()) == {"energy"}     # a kind with no rows is absent


@pytest.mark.parametrize("name", ["ragged0", "ragged1", "ties", "fences", "constant"])
def test_normalize_equals_get_prosody_bit_for_bit(st, gold, corpora, name):
    s = want_stats(gold, name)["energy"]
    x, lens = sc.batch(corpora[name], "energy")
    got = st.normalize(x, lens, s["mean"], s["std"])
    st.sync()
    got = got.cpu().numpy()
    flat = np.concatenate([got[b, :n] for b, n in enumerate(lens)])
    assert bits(flat) == bits(gold[f"{name}/energy/target"])
    assert all((got[b, n:] == 0).all() for b, n in enumerate(lens)) and np.array_equal(got, sr.normalize(x, lens, s["mean"], s["std"]))
    short = lens.copy()
    short[0] = 0
    again = st.normalize(x, short, s["mean"], s["std"])
    st.sync()
    assert (again[0] == 0).all().item() and np.array_equal(again[1:].cpu().numpy(), got[1:])
