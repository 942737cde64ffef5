"""What the host and the GPU tests of forced alignment share: the fixtures of tools/make_aligner_goldens.py, the bars, and the inputs a
fixture stands for (its weights are regenerated from the stored seed)."""
from e2e_tts_amd import aligner as al, synth_weights as sw

FORWARD_FIXTURES = ["aligner_tiny_b3", "aligner_tiny_noprior_b2", "aligner_tiny_wide_b1", "aligner_full_b2"]
MEAN_BAR, MAX_BAR = 4.0, 8.0   # x the reference's own |fp32 - float64| on the fixture (the denoiser tests' margin: summation order differs)


def fixture_state(g):
    return sw.make_aligner_state(int(g["hidden"]), int(g["n_mel"]), seed=int(g["weight_seed"]), weight_scale=float(g["weight_scale"]))


def fixture_inputs(g):
    """(submodule weights, keys [B, L, H], speaker vectors [B, H], prior or None) of a forward fixture."""
    state = fixture_state(g)
    keys = state["encoder.src_word_emb.weight"][g["ids"]]
    spk = state["speaker_emb.weight"][g["speakers"]]
    prior = None
    if int(g["has_prior"]):
        prior = g["prior"] if "prior" in g else al.batch_prior(g["txt_lens"], g["mel_lens"], g["mel"].shape[1], g["ids"].shape[1])
    return state, keys, spk, prior
