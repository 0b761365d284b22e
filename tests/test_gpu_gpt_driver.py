"""train_lang/pretrain_gpt_lang_model.py on the GPU: the synthetic corpus with a 2-layer decoder for a few steps (finite
losses, the token-driven schedule, a checkpoint that round-trips), and 20 steps on one fixed batch with dropout 0 ending
below the first loss."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_driver_round_trip(tmp_path):
    from train_lang import pretrain_gpt_lang_model as drv
    from vcg_hip.build import build_gpt_model
    from vcg_hip.nn import OpenAIGPTConfig
    ck_dir = tmp_path / "ck"
    tr = drv.main(["--epoch", "2", "--batch_size", "4", "--videos", "8", "--max_text_len", "32", "--n_layer", "2",
                   "--ckpt_path", str(ck_dir)])
    assert len(tr.history) == 4 and all(np.isfinite(h["loss"]) for h in tr.history)
    assert tr.history[0]["tokens"] > 0 and tr.history[-1]["tokens"] > tr.history[0]["tokens"]
    assert "pretrain_0.pth" in sorted(f.name for f in ck_dir.iterdir())
    ck = torch.load(str(ck_dir / "pretrain_0.pth"), map_location="cpu", weights_only=True)
    assert set(ck) == {"epoch", "best_loss", "model_state_dict", "optimizer_state_dict", "tokens"}
    assert ck["epoch"] == 0 and np.isfinite(ck["best_loss"])
    sd = ck["model_state_dict"]
    assert sd["head.weight"].shape == (40478, 768) and sd["base_model.h.1.attn.c_attn.weight"].shape == (768, 2304)
    # the checkpoint loads into a fresh model, and its decoder into transformers' layout (GPTHugface(checkpoint=))
    m = build_gpt_model(seed=5, precision="bf16", config=OpenAIGPTConfig(n_layer=2))
    m.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, sd[k]) for k, v in m.state_dict().items())
    opt = m.configure_optimizers(drv.TrainerConfig())
    opt.load_state_dict(ck["optimizer_state_dict"])


def test_fixed_batch_loss_goes_down():
    from data.synthetic_dataset import HashGPTTokenizer, SyntheticVideoCorpus
    from data.youtube_subtitle_dataset import SyntheticSubtitleDatasetForGPT
    from train_lang.pretrain_gpt_lang_model import TrainerConfig
    from vcg_hip.build import build_gpt_model
    from vcg_hip.nn import OpenAIGPTConfig
    import random
    random.seed(3)
    ds = SyntheticSubtitleDatasetForGPT(SyntheticVideoCorpus(4, H=8, W=8, seed=5), HashGPTTokenizer(), 16, 32)
    x, y, mask = (torch.stack(t).to(DEV) for t in zip(*[ds[i] for i in range(4)]))
    m = build_gpt_model(seed=123, device=DEV, precision="bf16", dropout=0.0, config=OpenAIGPTConfig(n_layer=2)).train()
    opt = m.configure_optimizers(TrainerConfig(learning_rate=1e-4))
    losses = []
    for _ in range(20):
        m.zero_grad()
        loss, _, n_valid = m.lm_loss(x, mask, y)
        assert n_valid > 0
        loss.backward()
        opt.clip_and_step(1.0)
        losses.append(loss.item())
    print("fixed-batch losses:", [round(v, 3) for v in losses[::4]], round(losses[-1], 3))
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
