"""Texts against BERT's position table, and the size of the fused attention's saved state.

BertModel (HF semantics, bert_hugface.py:20) indexes position_embeddings by token position, so a text longer than
config.max_position_embeddings has no embedding: HF fails on the lookup; the native embedding kernel would read past the
table, so BertModel raises before any launch. The fused attention keeps only per-query statistics
(vcg_bert_attn_stats_bytes): float2 [B*nh][128] at L <= 128, as the one-workgroup kernels always had."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "video-chapter-generation_amd"))


def _small_bert():
    from vcg_hip.nn import BertConfig, BertModel
    cfg = BertConfig(hidden_size=64, num_hidden_layers=1, num_attention_heads=1, intermediate_size=128,
                     max_position_embeddings=16)
    return BertModel(cfg)


@pytest.mark.parametrize("entry", ["forward", "native_forward"])
def test_text_longer_than_the_position_table_raises(entry, monkeypatch):
    from vcg_hip import _lib
    m = _small_bert()

    def no_library(*a, **k):
        raise AssertionError("the library was reached before the length check")
    monkeypatch.setattr(_lib, "lib", no_library)
    ids = torch.ones((2, 17), dtype=torch.int64)
    mask = torch.ones_like(ids)
    with pytest.raises(ValueError, match=r"17.*16"):
        if entry == "forward":
            m(input_ids=ids, attention_mask=mask)
        else:
            m.native_forward(ids, mask)


def test_driver_check_names_both_numbers():
    from vcg_hip.nn import check_max_text_len
    m = torch.nn.Sequential(_small_bert())
    check_max_text_len(m, 16)
    with pytest.raises(SystemExit, match=r"--max_text_len 17.*16 positions"):
        check_max_text_len(m, 17)


def test_stats_size_query():
    """L <= 128: the one-workgroup kernels' float2 [B*nh][128]; above it the sequence rounded up to the 128-row tile,
    float2 statistics plus the backward's float D per query. (The library loads without a GPU: the query is host code.)"""
    from vcg_hip import _lib
    q = lambda B, nh, L: _lib.query("vcg_bert_attn_stats_bytes", B, nh, L)
    for L in (1, 7, 100, 128):
        assert q(64, 12, L) == 64 * 12 * 128 * 8
    assert q(3, 12, 129) == 3 * 12 * 256 * 12
    assert q(3, 12, 256) == 3 * 12 * 256 * 12
    assert q(3, 12, 250) == 3 * 12 * 256 * 12
    assert q(2, 12, 512) == 2 * 12 * 512 * 12
    assert q(0, 12, 512) == 0
