"""CPU tests of teacher-forced scoring's host side (hip_models.gpt: score_inputs, score_reduce; GPT.score's checks): the layout of the scored
sequences and the target / row alignment, the loss and accuracy reduction against torch.nn.functional.cross_entropy + argmax, bad inputs."""
import pytest
import torch
import torch.nn.functional as F

from chatttsplus_amd.hip_models.gpt import _check_left_padded, score_inputs, score_reduce

EOS = 625


def _prompts(lens, T, seed=0):
    """Left-padded prompts as Tokenizer.encode gives them: ids [B, T, 4] (text ids replicated), mask, text_mask = mask."""
    g = torch.Generator().manual_seed(seed)
    B = len(lens)
    ids = torch.zeros(B, T, 4, dtype=torch.long)
    mask = torch.zeros(B, T, dtype=torch.long)
    for b, n in enumerate(lens):
        ids[b, T - n:] = torch.randint(700, 21000, (n, 1), generator=g).expand(n, 4)
        mask[b, T - n:] = 1
    return ids, mask, mask.bool()


def _codes(ns, seed=1):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 625, (n, 4), generator=g) for n in ns]


@pytest.mark.parametrize("append_eos", [True, False])
def test_score_inputs_layout_and_alignment(append_eos):
    lens, ns = [7, 3, 12], [5, 17, 1 if append_eos else 2]
    ids, mask, tm = _prompts(lens, 12)
    codes = _codes(ns)
    si = score_inputs(ids, mask, tm, codes, EOS, append_eos=append_eos)
    n_in = [n if append_eos else n - 1 for n in ns]
    T = max(p + c for p, c in zip(lens, n_in))
    assert si["ids"].shape == (3, T, 4) and si["mask"].shape == (3, T) and si["text_mask"].shape == (3, T)
    assert si["mask"].dtype == torch.int32 and si["text_mask"].dtype == torch.bool
    assert si["n_targets"].tolist() == [n + 1 if append_eos else n for n in ns]
    assert si["targets"].shape == (3, max(si["n_targets"].tolist()), 4)
    for b in range(3):
        L = lens[b] + n_in[b]
        assert si["mask"][b].tolist() == [0] * (T - L) + [1] * L                               # left padded again
        assert si["text_mask"][b].tolist() == [False] * (T - L) + [True] * lens[b] + [False] * n_in[b]
        assert torch.equal(si["ids"][b, T - L:T - n_in[b]], ids[b, 12 - lens[b]:])              # the prompt, unchanged
        assert torch.equal(si["ids"][b, T - n_in[b]:], codes[b][:n_in[b]])                      # the codes follow it
        nb = int(si["n_targets"][b])
        tg = si["targets"][b, :nb]
        assert torch.equal(tg[:ns[b]], codes[b].to(torch.int32))
        if append_eos:
            assert tg[-1].tolist() == [EOS] * 4
        # alignment: row T - n_b + j predicts target j, i.e. target j is the input row T - n_b + j + 1 wherever that row exists
        for j in range(nb - 1):
            assert torch.equal(si["ids"][b, T - nb + j + 1].to(torch.int32), tg[j]), (b, j)
        assert bool(si["mask"][b, T - nb:].all()), "a scored row is a pad"
        assert not bool(si["text_mask"][b, T - nb + 1:].any()), "a target row is a text row"


def test_score_reduce_matches_cross_entropy_and_argmax():
    g = torch.Generator().manual_seed(5)
    ns = [4, 9, 1]
    V = 626
    logits = [torch.randn(n, 4, V, generator=g) * 3 for n in ns]
    tg = [torch.randint(0, V, (n, 4), generator=g) for n in ns]
    tg[0][1, 2] = int(logits[0][1, 2].argmax())                    # some right answers
    tg[1][:, 0] = logits[1][:, 0].argmax(-1)
    lps = [torch.log_softmax(lg, -1).gather(-1, t[..., None])[..., 0] for lg, t in zip(logits, tg)]
    ams = [lg.argmax(-1) for lg in logits]
    nll, acc, loss, accuracy = score_reduce(lps, ams, tg)
    # train_lora.py:455-469 over the same entries: padded to one [B, n_max, 4] batch with IGNORE rows
    nmax = max(ns)
    big = torch.zeros(3, nmax, 4, V)
    lab = torch.full((3, nmax, 4), -100, dtype=torch.long)
    for b, n in enumerate(ns):
        big[b, :n] = logits[b]
        lab[b, :n] = tg[b]
    ce = F.cross_entropy(big.flatten(0, 2), lab.flatten(0, 2), ignore_index=-100)
    pred = big.flatten(0, 2).argmax(-1)
    lf = lab.flatten(0, 2)
    valid = lf != -100
    ref_acc = (pred[valid] == lf[valid]).float().mean()
    assert abs(loss - float(ce)) <= 1e-5 * max(1.0, abs(float(ce)))
    assert abs(accuracy - float(ref_acc)) <= 1e-7
    for b in range(3):
        assert abs(float(nll[b]) - float(F.cross_entropy(logits[b].flatten(0, 1), tg[b].flatten()))) <= 1e-5
        assert abs(float(acc[b]) - float((logits[b].argmax(-1) == tg[b]).float().mean())) <= 1e-7


def test_bad_inputs_raise():
    ids, mask, tm = _prompts([5, 3], 6)
    codes = _codes([4, 4])
    right = mask.flip(1)
    with pytest.raises(ValueError, match="LEFT padding"):
        score_inputs(ids, right, tm, codes, EOS)
    holed = mask.clone(); holed[0, 3] = 0
    with pytest.raises(ValueError, match="LEFT padding"):
        _check_left_padded(holed)
    with pytest.raises(ValueError, match="no token"):
        _check_left_padded(torch.zeros(2, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="code sequences"):
        score_inputs(ids, mask, tm, codes[:1], EOS)
    with pytest.raises(ValueError, match=r"\[n, 4\]"):
        score_inputs(ids, mask, tm, [codes[0], codes[1][:, :3]], EOS)
    with pytest.raises(ValueError, match="nothing to score"):
        score_inputs(ids, mask, tm, [codes[0], codes[1][:0]], EOS, append_eos=False)
    with pytest.raises(ValueError):
        score_inputs(ids[..., 0], mask, tm, codes, EOS)
