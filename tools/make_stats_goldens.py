"""Writes tests/golden/stats_cases.npz: what the reference's own text computes on the seeded corpora of tests/stats_cases.py.

The reference's data loader cannot be imported here (its imports need parselmouth, pyworld and librosa), so the text of three
functions is extracted with ``ast`` and executed with numpy / sklearn / tqdm, as tools/make_forced_goldens.py does for ``get_f0``:
``remove_outlier`` (src/tools/utils.py:142-150), ``TextMelLoader.build_stats`` (src/tools/dataloader.py:106-151) and
``TextMelLoader.get_prosody`` (dataloader.py:179-183).  A stand-in ``self`` carries ``inputs`` and ``prosody_path`` pointing at temporary
.npy files.  None of the reference's text is written anywhere.

Per corpus ``c`` the fixture holds: ``c/digest`` (sha256 of the rows: the generator has not drifted), for kind in energy, pitch
``c/<kind>/p25 | p75 | lower | upper`` float32 [rows] and ``c/<kind>/kept`` int64 [rows] -- the locals of ``remove_outlier``'s body, run
statement by statement on each row --, ``c/stats`` float64 [10] (build_stats' dict in the order of stats_cases.STAT_KEYS) and, for the
small corpora, ``c/energy/target``: ``get_prosody``'s rows, concatenated, with that dict as ``self.stats``.

Run from the repository root with the reference checkout beside it (oracle/make_goldens.py: REF)."""
from __future__ import annotations

import ast
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stats_cases as sc  # noqa: E402

TARGET_CORPORA = ("ragged0", "ragged1", "ties", "fences", "constant")   # whose get_prosody rows are stored (no row of the cap's length)


def reference_functions():
    """-> (namespace holding remove_outlier / build_stats / get_prosody, the statements of remove_outlier's body before its return)."""
    import tqdm
    import torch
    from sklearn.preprocessing import StandardScaler
    from oracle.make_goldens import REF
    ns = {"np": np, "os": os, "tqdm": tqdm, "torch": torch, "StandardScaler": StandardScaler}
    utils = ast.parse(open(os.path.join(REF, "e2e_tts", "src", "tools", "utils.py")).read())
    ro = next(n for n in utils.body if isinstance(n, ast.FunctionDef) and n.name == "remove_outlier")
    loader = ast.parse(open(os.path.join(REF, "e2e_tts", "src", "tools", "dataloader.py")).read())
    methods = [n for c in loader.body if isinstance(c, ast.ClassDef) and c.name == "TextMelLoader" for n in c.body
               if isinstance(n, ast.FunctionDef) and n.name in ("build_stats", "get_prosody")]
    assert len(methods) == 2
    exec(compile(ast.Module(body=[ro] + methods, type_ignores=[]), "reference", "exec"), ns)
    body = [s for s in ro.body if not isinstance(s, ast.Return)]
    return ns, compile(ast.Module(body=body, type_ignores=[]), "remove_outlier", "exec")


def main():
    ns, ro_body = reference_functions()
    arrays = {}
    tmp = tempfile.mkdtemp()
    mel = os.path.join(tmp, "mel.npy")
    np.save(mel, np.zeros((1, 1), np.float32))
    for cname, utts in sc.corpora().items():
        inputs, paths = [], {}
        rows = {k: {f: [] for f in ("p25", "p75", "lower", "upper", "kept")} for k in ("energy", "pitch")}
        for i, u in enumerate(utts):
            wav = os.path.join(tmp, f"{cname}_{i}.wav")
            inputs.append((wav, "spk"))
            entry = {"mel": mel}
            for k in ("energy", "pitch", "f0"):
                entry[k] = os.path.join(tmp, f"{cname}_{i}_{k}.npy")
                # energy and pitch as the float32 frames they are; f0 in float64, the dtype np.mean / np.std run in per the definition
                np.save(entry[k], u[k] if k != "f0" else u[k].astype(np.float64))
            paths["_".join(["spk", os.path.basename(wav)])] = entry
            for k in ("energy", "pitch"):
                scope = {"np": np, "in_dir": entry[k]}
                exec(ro_body, scope)                       # remove_outlier's own statements: its locals are the row's figures
                kept = ns["remove_outlier"](entry[k])
                assert len(kept) == int(scope["normal_indices"].sum())
                for f in ("p25", "p75", "lower", "upper"):
                    assert scope[f].dtype == np.float32
                    rows[k][f].append(scope[f])
                rows[k]["kept"].append(len(kept))
        me = types.SimpleNamespace(inputs=inputs, prosody_path=paths)
        stats = ns["build_stats"](me)
        arrays[f"{cname}/stats"] = np.array([stats[k.split(".")[0]][k.split(".")[1]] for k in sc.STAT_KEYS], np.float64)
        arrays[f"{cname}/digest"] = sc.digest(utts)
        for k in ("energy", "pitch"):
            for f in ("p25", "p75", "lower", "upper"):
                arrays[f"{cname}/{k}/{f}"] = np.array(rows[k][f], np.float32)
            arrays[f"{cname}/{k}/kept"] = np.array(rows[k]["kept"], np.int64)
        if cname in TARGET_CORPORA:
            me.stats = stats
            t = [ns["get_prosody"](me, name, "energy").numpy() for name in paths]
            assert all(x.dtype == np.float32 for x in t)
            arrays[f"{cname}/energy/target"] = np.concatenate(t)
        print(f"[{cname}] {len(utts)} utterances: {stats}", flush=True)
    os.makedirs(os.path.dirname(sc.GOLD), exist_ok=True)
    np.savez_compressed(sc.GOLD, **arrays)
    print(f"-> {sc.GOLD}: {os.path.getsize(sc.GOLD) / 1024:.0f} KiB", flush=True)


if __name__ == "__main__":
    main()
