"""Per-utterance and per-phoneme controls, host side (CPU, -m "not gpu"): the binding's shape handling (_lib.control_array), the
routing of per-text speakers and controls through TTS's batching (TTS.plan_requests), and the numpy oracle against the fixtures the
reference produced with tensor controls (tools/make_ctl_goldens.py)."""
import numpy as np
import pytest

from conftest import load_golden, states_for
from e2e_tts_amd import config as cfgmod
from e2e_tts_amd._lib import control_array
from e2e_tts_amd.api import TTS
from oracle import ref_numpy as orc

B, L = 3, 5


@pytest.mark.parametrize("shape,uv,n", [
    ((B, 1), False, B), ((B, L), False, B * L), ((1, L), False, B * L), ((L,), False, B * L), ((1, 1), False, 1), ((1,), False, 1),
    ((), False, 1), ((B, 1, 1), True, B), ((B, L, 1), True, B * L), ((1, L, 1), True, B * L), ((L, 1), True, B * L), ((1,), True, 1)])
def test_broadcast_shapes_materialise_to_the_right_count_and_layout(shape, uv, n):
    import torch
    x = np.asarray(np.arange(1, 1 + int(np.prod(shape)), dtype=np.float64).reshape(shape) / 8)
    full = np.broadcast_to(x, (B, L, 2) if uv else (B, L)).astype(np.float32)   # what the reference multiplies with
    full = full[..., 0] if uv else full
    for arg in (x, torch.from_numpy(x)):
        v, count = control_array(arg, B, L, uv_pitch=uv)
        assert count == n
        v = np.asarray(v)
        assert v.dtype == np.float32 and v.size == n and v.flags["C_CONTIGUOUS"]
        if n == B * L:
            np.testing.assert_array_equal(v.reshape(B, L), full)
        elif n == B:
            np.testing.assert_array_equal(v, full[:, 0])
        else:
            assert (full == v[0]).all()


def test_numbers_stay_scalars():
    for x in (1, 0.8, np.float32(1.25), np.float64(0.5)):
        v, f = control_array(x, B, L)
        assert v is None and f == float(x)


@pytest.mark.parametrize("shape,uv", [((B, L, 2), True), ((B, 1, 2), True), ((B, L), True), ((2, L), False), ((B, L + 1), False),
                                      ((B, L, 1), False), ((1, B, L), False), ((B, L, 1, 1), True), ((L + 1,), False)])
def test_unsupported_shapes_raise_value_error(shape, uv):
    with pytest.raises(ValueError):
        control_array(np.ones(shape, np.float32), B, L, uv_pitch=uv)


def _texts():
    # "aaa , bbb , ..." lines longer than 1.5 x max_len are cut into pieces (arrange_text, reference API/utils.py:64-80)
    long_a = " , ".join("a" * 9 for _ in range(6))
    long_b = " , ".join("b" * 7 for _ in range(5))
    return ["c" * 12, long_a, "d" * 5, long_b, "e" * 12]


def test_arrange_text_owners_follow_every_piece():
    texts = _texts()
    pieces, owners = TTS.arrange_text_owners(texts, 20)
    assert len(pieces) > len(texts)
    assert pieces == TTS.arrange_text_owners(texts, 20)[0]
    for p, o in zip(pieces, owners):
        assert set(p.replace(" , ", "")) == set(texts[o].replace(" , ", ""))   # each text's letters are its own
    assert owners == sorted(owners)


def test_per_text_entries_land_on_their_rows_after_split_sort_and_revert():
    texts = _texts()
    pieces, owners = TTS.arrange_text_owners(texts, 20)
    seqs = [[4 + (ord(c) % 127) for c in p] for p in pieces]
    spk_t = [0, 1, 2, 3, 1]
    d_t, p_t, e_t = [1.0, 0.7, 1.3, 0.9, 1.1], [0.6, 1.2, 1.0, 1.5, 0.8], [1.4, 0.5, 0.9, 1.0, 1.2]
    follow = lambda v: [v[o] for o in owners]   # noqa: E731 -- what TTS.inference hands inference_ids
    plan, revert = TTS.plan_requests(seqs, 20, follow(spk_t), follow(d_t), follow(p_t), follow(e_t))
    batches, revert_ref = TTS.pack_sequences(seqs, 20)
    np.testing.assert_array_equal(revert, revert_ref)
    assert len(plan) == len(batches) >= 2
    seen = []
    for item, (ids, lens) in zip(plan, batches):
        np.testing.assert_array_equal(item["ids"], ids)
        np.testing.assert_array_equal(item["lens"], lens)
        rows = list(item["rows"])
        seen += rows
        for r, j in enumerate(rows):   # row r of this batch IS sequence j, and carries the entries of j's text
            np.testing.assert_array_equal(ids[r, :len(seqs[j])], seqs[j])
            o = owners[j]
            spk = item["speaker"]
            assert int(spk[r] if spk.size > 1 else spk[0]) == spk_t[o]
            for key, ref in (("duration_control", d_t), ("pitch_control", p_t), ("energy_control", e_t)):
                v = item[key]
                got = float(v) if np.ndim(v) == 0 else float(np.asarray(v)[r, 0])
                assert got == np.float32(ref[o]), (key, r, j)
    # the batches' rows in order, reverted, give the sequences back in input order
    assert [seen[i] for i in revert] == list(range(len(seqs)))


def test_all_equal_lists_plan_exactly_what_scalars_plan():
    rng = np.random.Generator(np.random.PCG64(3))
    seqs = [list(rng.integers(4, 131, n)) for n in (25, 9, 31, 31, 14, 3)]
    a, ra = TTS.plan_requests(seqs, 60, 2, 1.1, 0.9, 1.2)
    b, rb = TTS.plan_requests(seqs, 60, [2] * 6, [1.1] * 6, [0.9] * 6, [1.2] * 6)
    np.testing.assert_array_equal(ra, rb)
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x.keys() == y.keys()
        for k in x:
            assert type(x[k]) is type(y[k]), k
            np.testing.assert_array_equal(x[k], y[k])


def test_per_phoneme_entries_and_mixed_batches():
    seqs = [[5] * 4, [6] * 2, [7] * 3]
    ph = np.array([0.5, 0.75, 1.0], np.float32)
    plan, _ = TTS.plan_requests(seqs, 100, 0, [1.0, 1.2, ph], 1.0, [0.8, 0.8, 0.8])
    (item,) = plan
    assert item["energy_control"] == np.float32(0.8) and item["pitch_control"] == 1.0
    d = item["duration_control"]
    assert d.shape == (3, 4) and d.dtype == np.float32
    np.testing.assert_array_equal(d[0], [1.0] * 4)                 # sequence 0 (longest) is row 0
    np.testing.assert_array_equal(d[1], [0.5, 0.75, 1.0, 1.0])     # sequence 2, padded with its last value
    np.testing.assert_array_equal(d[2], [np.float32(1.2)] * 4)
    with pytest.raises(ValueError):
        TTS.plan_requests(seqs, 100, 0, [1.0, 1.0, np.ones(4)])     # per-phoneme entry of the wrong length
    with pytest.raises(ValueError):
        TTS.plan_requests(seqs, 100, [0, 1])                        # one entry short


CTL_CASES = ["tiny_pctl_b3", "tiny_nouv_pctl_b3", "tiny_frame_pctl_b3"]


def mean_l1(a, b):
    return float(np.abs(a.astype(np.float64) - b.astype(np.float64)).mean())


@pytest.mark.parametrize("name", CTL_CASES)
def test_oracle_with_array_controls_reproduces_the_reference_fixtures(name):
    g = load_golden(name)
    cfg, ac_state, voc_state = states_for(g, name)
    ac = orc.AcousticOracle(ac_state, cfg, cfgmod.DEFAULT_STATS)
    (mel, mel_post, dur), mel_lens = ac.inference(np.array([int(g["speaker"])]), g["ids"], g["lens"], g["d_control"], g["p_control"],
                                                  g["e_control"])
    np.testing.assert_array_equal(dur, g["dur"])
    np.testing.assert_array_equal(mel_lens, g["mel_lens"])
    np.testing.assert_array_equal(ac.trace["pitch_idx"], g["pitch_idx"])
    np.testing.assert_array_equal(ac.trace["energy_idx"], g["energy_idx"])
    assert mean_l1(ac.trace["log_d"], g["log_d"]) < 1e-5
    assert mean_l1(ac.trace["pitch_pred"], g["pitch_pred"]) < 1e-5
    assert mean_l1(mel, g["mel"]) < 1e-5
    assert mean_l1(mel_post, g["mel_post"]) < 1e-5
    wav = orc.VocoderOracle(voc_state, cfg).forward(g["mel_post"].transpose(0, 2, 1))[:, 0]
    assert mean_l1(wav, g["wav"]) < 1e-5
    # the controls really vary per phoneme, and they moved decisions away from what the unit controls give
    assert np.unique(g["d_control"]).size > 1 and 0.5 <= g["d_control"].min() and g["d_control"].max() <= 1.6
    (_, _, dur1), _ = ac.inference(np.array([int(g["speaker"])]), g["ids"], g["lens"])
    assert not np.array_equal(dur1, g["dur"])


def test_frame_level_fixture_expands_per_phoneme_controls_along_the_durations():
    """tiny_frame_pctl_b3 stores the [B, L] arrays the engine takes and the [B, T] ones the reference got: the second is the first
    expanded by the rule of include/e2etts.h (frame t -> phoneme covering it, past mel_len -> the row's last phoneme)."""
    g = load_golden("tiny_frame_pctl_b3")
    T = g["mel"].shape[1]
    cum = np.cumsum(g["dur"].astype(np.int64), axis=1)
    Lp = g["ids"].shape[1]
    for ph, fr in (("p_control_ph", g["p_control"][..., 0]), ("e_control_ph", g["e_control"])):
        assert fr.shape == (len(g["lens"]), T)
        for b in range(fr.shape[0]):
            for t in range(T):
                i = min(int(np.sum(cum[b] <= t)), Lp - 1)
                assert fr[b, t] == g[ph][b, i]
