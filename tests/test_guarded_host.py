"""tests/guarded.py on host memory: the helper itself must notice what it is there to notice — a store
one element before or behind a buffer, an element never written, a gap element written, a modified input —
and must accept the engine's own canonical NaN as a written value."""
import numpy as np
import pytest
import torch

from guarded import BAND, SENTINEL, Guarded


def build(misalign=False):
    gb = Guarded(device="cpu", misalign=misalign)
    gb.inp("gamma", np.linspace(0.0, 1.0, 11)).inp("runs", np.arange(5, dtype=np.int64))
    gb.out("w", (7, 3)).out("cost", (7,)).out("status", (7,), torch.int8).out("perm", (7,), torch.int64)
    return gb.build()


@pytest.mark.parametrize("misalign", [False, True])
def test_layout_and_patterns(misalign):
    gb = build(misalign)
    for name in ("gamma", "w", "cost", "runs", "perm"):
        assert gb.ptr(name) % 16 == (8 if misalign else 0)
    assert gb.view("w").shape == (7, 3) and gb.ptr("nothing") is None
    spans = sorted((a, n) for dt, a, n in gb._at.values() if dt == torch.float64)
    assert spans[0][0] >= BAND and all(b[0] - (a[0] + a[1]) >= BAND for a, b in zip(spans, spans[1:]))
    assert gb._arena[torch.float64].numel() - (spans[-1][0] + spans[-1][1]) >= BAND
    gb.check_bands()
    gb.check_inputs()
    for name in ("w", "cost", "status", "perm"):
        gb.check_untouched(name)
        with pytest.raises(AssertionError):
            gb.check_written(name)
    assert np.isnan(gb.np("w")).all() and SENTINEL[torch.float64] != torch.tensor(float("nan")).double().view(torch.int64).item()
    gb.view("w").fill_(float("nan"))  # the canonical NaN (an invalid EV's row) counts as written
    gb.check_written("w")


@pytest.mark.parametrize("name,dtype", [("w", torch.float64), ("status", torch.int8), ("perm", torch.int64)])
@pytest.mark.parametrize("side", [-1, 1])
def test_stray_store_is_seen(name, dtype, side):
    gb = build()
    _, a, n = gb._at[name]
    gb._arena[dtype][a - 1 if side < 0 else a + n] = 0
    with pytest.raises(AssertionError, match="band"):
        gb.check_bands()


def test_masks_and_inputs():
    gb = build()
    rows = np.array([True, True, False, True, True, False, False])
    gb.view("cost")[torch.as_tensor(rows)] = 1.0
    gb.check_written("cost", rows)
    with pytest.raises(AssertionError, match="never written"):
        gb.check_written("cost", ~rows | rows)
    gb.view("cost")[2] = 0.0
    with pytest.raises(AssertionError, match="gap"):
        gb.check_written("cost", rows)
    gb.view("w")[rows] = 0.5
    gb.check_written("w", rows[:, None])
    gb.check_inputs()
    gb.view("gamma")[3] = np.nextafter(gb.view("gamma")[3].item(), 2.0)
    with pytest.raises(AssertionError, match="input gamma"):
        gb.check_inputs()
