"""train_chapter_title_gen.py's Trainer on the GPU: the tiny config of tests/test_gpu_pegasus_model.py, the corpus of
tests/title_corpus_util.py, the stub tokenizer and dropout 0, for a few epochs (no test split: a checkpoint per epoch).

  * the mean training loss of the last epoch is below the first epoch's;
  * a checkpoint per epoch and the checkpoint_best.pth link to the last one are written;
  * PegasusHugface(checkpoint=that file) -- the `base_model.` prefix path -- reproduces the trained model's title_loss
    bit for bit, and generate_ids runs on it;
  * two runs from the same seed write identical weights.
"""
import os

import numpy as np
import pytest
import torch

import title_corpus_util as tc
from test_gpu_pegasus_model import CFG

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPOCHS, L, T = 8, 40, 8


@pytest.fixture(scope="module", autouse=True)
def _init():
    from vcg_hip import _lib
    _lib.call("vcg_init", 0)


def _config():
    from vcg_hip.nn import PegasusConfig
    return PegasusConfig(**dict(CFG, dropout=0.0, attention_dropout=0.0, activation_dropout=0.0))


def _train(root, seed):
    import train_chapter_title_gen as drv
    from common_utils import set_random_seed
    from data.synthetic_dataset import HashPegasusTokenizer
    from data.youtube_chapter_title_dataset import YoutubeChapterTitleDataset
    from model.lang.pegasus_hugface import PegasusHugface
    os.makedirs(root)
    data_file, vid_file = tc.write_title_corpus(os.path.join(root, "corpus"))
    set_random_seed.use_fix_random_seed(seed)
    model = PegasusHugface(reinit_head=True, config=_config()).to(DEV)
    model.precision = "bf16"
    tok = HashPegasusTokenizer(CFG["vocab_size"])
    ds = YoutubeChapterTitleDataset(data_file, vid_file, tok, max_text_len=L, chapter_title_text_len=T)
    conf = drv.TrainerConfig(max_epochs=EPOCHS, batch_size=2, learning_rate=1e-3, ckpt_dir=os.path.join(root, "ck"))
    tr = drv.Trainer(model, tok, ds, None, conf)
    tr.device = torch.device(DEV)
    tr.train()
    torch.cuda.synchronize()
    return tr, ds


def test_driver_trains_saves_and_reloads(tmp_path):
    from model.lang.pegasus_hugface import PegasusHugface
    tr, ds = _train(str(tmp_path / "a"), 7)
    losses = [h["loss"] for h in tr.history]
    print("training loss per epoch:", [round(v, 3) for v in losses])
    assert len(losses) == EPOCHS and all(np.isfinite(losses)) and losses[-1] < losses[0]
    ck = tmp_path / "a" / "ck"
    names = sorted(p.name for p in ck.iterdir())
    assert len(names) == EPOCHS + 1 and "checkpoint_best.pth" in names and f"checkpoint_{EPOCHS}_-inf.pth" in names
    link = ck / "checkpoint_best.pth"
    assert os.path.islink(link) and os.path.realpath(link) == os.path.realpath(ck / f"checkpoint_{EPOCHS}_-inf.pth")
    sd = torch.load(str(link), map_location="cpu", weights_only=True)
    assert set(sd) == {"epoch", "best_result", "model_state_dict", "optimizer_state_dict"} and sd["epoch"] == EPOCHS
    assert all(k.startswith("base_model.") for k in sd["model_state_dict"])

    # the saved state through PegasusHugface(checkpoint=...): the same title_loss, bit for bit
    import random
    random.seed(3)
    batch = [torch.stack(t).to(DEV) for t in zip(*[ds[i] for i in range(len(ds))])]
    m2 = PegasusHugface(reinit_head=True, checkpoint=str(link), config=_config()).to(DEV)
    m2.precision = "bf16"
    out = []
    for m in (tr.model.eval(), m2.eval()):
        with torch.no_grad():
            loss, n_correct, n_valid = m.title_loss(*batch)
        out.append((loss.cpu(), int(n_correct), n_valid))
    assert torch.equal(out[0][0].view(torch.int32), out[1][0].view(torch.int32)) and out[0][1:] == out[1][1:]
    tokens, lengths = m2.generate_ids(batch[0], batch[1], max_len=5)
    assert tokens.shape[0] == len(ds) and tokens.shape[1] <= 5 and bool((lengths >= 1).all())

    # the same seed again: identical weights
    tr2, _ = _train(str(tmp_path / "b"), 7)
    a, b = tr.model.state_dict(), tr2.model.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert [h["loss"] for h in tr2.history] == losses
