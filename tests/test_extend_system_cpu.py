"""CPU: the host-side pieces of the extension features of System -- where an mmu prompt row splits into [.. image block | question tail]
(textproc.image_block_split, on the tiny tokenizer) and t0 of prefill_forced_prefix (System.forced_prefix_len)."""
import pytest
import torch

from plangen_amd.system import System
from plangen_amd.textproc import IMAGE_END_TAG, IMAGE_TAG, TagWordCodec, image_block_split, wrap_mmu_prompt_ids


def _codec():
    return TagWordCodec(512, eos_id=7, pad_id=3)


def test_split_column_is_behind_the_image_block_whatever_the_question():
    codec = _codec()
    P = 5
    end = codec.token_id(IMAGE_END_TAG)
    rows = [wrap_mmu_prompt_ids(codec, q, P) for q in ("where is the cat", "count the dogs on the mat please")]
    splits = []
    for _, ids, seq in rows:
        s = image_block_split(seq, ids, end)
        assert sum(seq) == P and all(seq[s - 1 - P:s - 1]) and ids[s - 1] == end and not any(seq[s:])
        assert image_block_split(seq) == s - 1                     # without the ids: one past the last image slot
        splits.append(s)
    (_, a, _), (_, b, _) = rows
    assert splits[0] == splits[1] and a[:splits[0]] == b[:splits[1]]      # the prefix does not depend on the question ...
    assert a[splits[0]:] != b[splits[1]:] and len(a) > splits[0]          # ... the tail does, and is never empty
    # left padding moves the column with the row
    pad = 4
    assert image_block_split([False] * pad + rows[0][2], [3] * pad + rows[0][1], end) == splits[0] + pad
    assert codec.token_id(IMAGE_TAG) in a[:splits[0]]


def test_split_column_needs_an_image_slot():
    with pytest.raises(ValueError):
        image_block_split([False, False, False])


def test_forced_prefix_len():
    g, B = 8, 3
    T = g * g
    assert System.forced_prefix_len(torch.zeros(B, g, g)) == T              # nothing edited: every token is forced
    r = torch.zeros(B, T); r[1, 0] = 1
    assert System.forced_prefix_len(r) == 0                                  # a region that starts at cell 0: nothing to prefill
    r = torch.zeros(B, T); r[0, 40:] = 1; r[1, 17] = 1; r[2, 63] = 1
    assert System.forced_prefix_len(r) == 17                                 # the batch minimum
    assert System.forced_prefix_len(r.view(B, g, g)) == 17                   # [B, g, g] and [B, T] alike
    assert System.forced_prefix_len(r[:1]) == 40
    r = -torch.ones(1, T); r[0, :5] = 0
    assert System.forced_prefix_len(r) == 5                                  # != 0, not > 0
