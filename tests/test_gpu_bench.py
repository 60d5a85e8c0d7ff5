"""bench.py on the GPU at micro dims: a plain run's line and its --dump-outputs files."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ARGS = ["--gpus", "1", "--model", "micro-test", "--batch", "3", "--lanes", "2", "--max-length", "24",
        "--steps", "3", "--warmup", "1"]


def _run(capsys, extra):
    import bench
    bench.main(ARGS + extra)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_bench_line_and_dump_are_reproducible(capsys, tmp_path):
    """A plain run prints the headline line only (no --full leg), --steps sets the timed
    steps, and two runs with the same arguments dump identical outputs: same seeded
    clips and weights in, the same ids and log-probabilities out, bit for bit."""
    a, b = tmp_path / "a", tmp_path / "b"
    la = _run(capsys, ["--dump-outputs", str(a)])
    _run(capsys, ["--dump-outputs", str(b)])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in la
    assert la["steps"] == 3 and la["full"] is False
    assert abs(la["value"] - 3 * 30.0 / (la["ms_per_step"] / 1e3)) / la["value"] < 0.01
    for k in ("roofline", "latency_b1", "beam5", "realistic_lengths", "streaming", "rest_mixed", "cpu_baseline"):
        assert k not in la
    names = sorted(f.name for f in a.iterdir())
    assert names == ["language.npy", "n_tokens.npy", "no_speech_prob.npy", "sum_logprob.npy", "tokens.npy"]
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype == np.float32 and np.array_equal(x, y), n
    tok, nt = np.load(a / "tokens.npy"), np.load(a / "n_tokens.npy")
    assert tok.shape == (3, 448) and (nt > 0).all()
    for i in range(3):
        assert (tok[i, :int(nt[i])] >= 0).all() and (tok[i, int(nt[i]):] == -1).all()
    assert np.isfinite(np.load(a / "sum_logprob.npy")).all()
