"""Generate tests/golden/mlm_masking.json: outputs of the REFERENCE masked-LM dataset class.

The reference module `data/youtube_subtitle_dataset.py` cannot be imported whole where torchvision, matplotlib and
scipy are missing (module-level imports its MLM class never uses). So, as tools/oracle/make_golden_datasets.py does,
the script parses the module with `ast` and executes only the class definition
`YoutubeClipSubtitleDatasetForHugFace` (:248-408) -- the reference's own code, unmodified -- in a namespace holding
the real modules it uses (torch, numpy, glob, random, os, json), the reference's own `data/common_utils.py` functions
(loaded by path) and its two padding constants. Nothing is stubbed.

Inputs: the CSV and subtitle JSONs of tests/corpus_util.py's corpus and data.synthetic_dataset.HashTokenizer. Python's
`random` is seeded before each item, as the tests do. The class opens the subtitle file before drawing, draws the clip
centre, then masks: one seed pins both draws.

Usage: python tools/oracle/make_golden_mlm.py <path to the reference's video_chapter_generation directory>
"""
import ast
import glob
import importlib.util
import json
import os
import random
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "video-chapter-generation_amd"), os.path.join(REPO, "tests"), REPO):
    sys.path.insert(0, p)

NAME = "YoutubeClipSubtitleDatasetForHugFace"
CONFIGS = [(16, 24), (16, 50), (8, 12), (32, 64)]  # (clip_frame_num, max_text_len): truncated, padded, short, and
# long enough (>= 6 masks) for the replacement draw
SEEDS = (1, 2, 3, 4, 5, 6)


def ref_class(ref):
    spec = importlib.util.spec_from_file_location("ref_common_utils", os.path.join(ref, "data", "common_utils.py"))
    cu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cu)
    ns = {"torch": torch, "np": np, "glob": glob, "random": random, "os": os, "json": json, "X_PAD": 0, "Y_PAD": -1,
          "parse_csv_to_list": cu.parse_csv_to_list, "extract_timestamp": cu.extract_timestamp}
    path = os.path.join(ref, "data", "youtube_subtitle_dataset.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    pads = sorted(ast.unparse(n) for n in tree.body if isinstance(n, ast.Assign) and
                  ast.unparse(n).startswith(("X_PAD", "Y_PAD")))
    assert pads == ["X_PAD = 0", "Y_PAD = -1"], pads  # (the module's constants are the ones given above)
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == NAME]
    assert len(nodes) == 1
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns[NAME]


def main():
    import corpus_util as cu
    from data.synthetic_dataset import HashTokenizer
    cls = ref_class(sys.argv[1])
    tok = HashTokenizer()
    out = {"source": f"reference data/youtube_subtitle_dataset.py {NAME} (ast-extracted, unmodified) run on "
                     "tests/corpus_util.py's corpus with data.synthetic_dataset.HashTokenizer", "configs": []}
    with tempfile.TemporaryDirectory() as root:
        _, data_file, vid_file, _, _, _ = cu.write_corpus(root, hw=8)
        for T, L in CONFIGS:
            ds = cls(data_file, vid_file, "bert", tok, clip_frame_num=T, max_text_len=L)
            items = []
            for seed in SEEDS:
                for i in range(len(ds)):
                    random.seed(seed)
                    x, y, m = ds[i]
                    items.append({"seed": seed, "i": i, "ids": x.tolist(), "targets": y.tolist(), "mask": m.tolist()})
            out["configs"].append({"clip_frame_num": T, "max_text_len": L, "items": items})
    path = os.path.join(REPO, "tests", "golden", "mlm_masking.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print("wrote", path, [len(c["items"]) for c in out["configs"]])


if __name__ == "__main__":
    main()
