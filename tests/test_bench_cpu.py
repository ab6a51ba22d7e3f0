"""Host logic of the bench line (no GPU): which figure becomes `value` of a multi-rank line."""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _line():
    return {"value": 2400.0, "ms_per_step": 1 / 2.4, "unit": "steps/s", "steps": 20, "energy_per_particle": -5.56, "kT_final": 0.98,
            "particle_steps_per_s": 2400.0 * 131072, "config": {"global_particles": 131072},
            "graph_variant": {"skipped": "transport 'native' is not available"},
            "graph_variant_peer": {"value": 8200.0, "ms_per_step": 1 / 8.2, "steps": 20, "energy_per_particle": -5.57, "kT": 0.985,
                                   "particles": 131072, "halo": {"transport": "peer"}}}


def test_a_verified_replay_becomes_the_value_and_the_eager_figure_stays():
    from benchlib import multirank
    d = multirank.promote_verified(_line())
    assert d["value"] == 8200.0 and d["eager"]["value"] == 2400.0 and "graph_variant_peer" in d["value_path"]
    assert abs(d["particle_steps_per_s"] - 8200.0 * 131072) < 1e-6 and abs(d["eager"]["particle_steps_per_s"] - 2400.0 * 131072) < 1e-6
    assert abs(d["ms_per_step"] - 1 / 8.2) < 1e-12


def test_a_replay_that_does_not_match_is_not_promoted():
    from benchlib import multirank
    for change in ({"kT": 1.3}, {"energy_per_particle": -4.9}, {"steps": 25}, {"value": 2000.0}, {"kT": float("nan")}):
        line = _line()
        line["graph_variant_peer"].update(change)
        d = multirank.promote_verified(copy.deepcopy(line))
        assert d["value"] == 2400.0 and "eager" not in d and d["value_path"].startswith("eager loop"), change
    line = _line()
    line["graph_variant_peer"] = {"skipped": "a phase timed out"}
    d = multirank.promote_verified(line)
    assert d["value"] == 2400.0 and "eager" not in d


def test_the_faster_of_two_verified_replays_wins():
    from benchlib import multirank
    line = _line()
    line["graph_variant"] = dict(line["graph_variant_peer"], value=9100.0, ms_per_step=1 / 9.1, halo={"transport": "native"})
    d = multirank.promote_verified(line)
    assert d["value"] == 9100.0 and "'native'" in d["value_path"]


def test_dumped_outputs_stay_within_the_limit_as_one_seeded_sample(tmp_path, monkeypatch):
    """--dump-outputs: arrays as written while they fit; past the limit every array keeps the SAME seeded rows, in order."""
    import numpy as np
    import torch
    from benchlib import md
    f = torch.randn((1000, 4), dtype=torch.float32)
    p = torch.randn((1000, 3), dtype=torch.float64)
    md.dump_outputs(str(tmp_path / "all"), {"force": f, "position": p})
    assert sorted(x.name for x in (tmp_path / "all").iterdir()) == ["force.npy", "position.npy"]
    assert np.array_equal(np.load(tmp_path / "all" / "force.npy"), f.numpy())
    monkeypatch.setattr(md, "DUMP_LIMIT_BYTES", 40000)
    for d in ("s1", "s2"):
        md.dump_outputs(str(tmp_path / d), {"force": f, "position": p})
    assert sum(x.stat().st_size for x in (tmp_path / "s1").iterdir()) <= 40000
    rows = np.load(tmp_path / "s1" / "sample_rows.npy")
    assert rows.dtype == np.float64 and 0 < len(rows) < 1000 and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(tmp_path / "s2" / "sample_rows.npy"))
    r = rows.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "s1" / "force.npy"), f.numpy()[r])
    assert np.array_equal(np.load(tmp_path / "s1" / "position.npy"), p.numpy()[r])
