"""Generate tests/golden/gpt_dataset.json: outputs of the REFERENCE dataset class with model_type "gpt".

As tools/oracle/make_golden_mlm.py does, the script parses the reference module `data/youtube_subtitle_dataset.py` with
`ast` and executes only the class definition `YoutubeClipSubtitleDatasetForHugFace` (:248-408) -- the reference's own
code, unmodified -- in a namespace holding the real modules it uses (torch, numpy, glob, random, os, json) and the
reference's own `data/common_utils.py` functions (loaded by path). The reference is read at run time only; nothing of
it is written anywhere but the recorded items.

Inputs: tests/corpus_util.py's corpus writer (two videos of 40 and 57 frames) and
data.synthetic_dataset.HashGPTTokenizer (a deterministic stub: ids in [0, 40478)). Python's `random` is seeded before
each item, as the tests do. max_text_len 6 truncates, 50 (the reference's) pads most items, 200 pads every item.

Usage: python tools/oracle/make_golden_gpt.py <path to the reference's video_chapter_generation directory>
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
CONFIGS = [(16, 50), (4, 6), (10, 200)]  # (clip_frame_num, max_text_len)
SEEDS = (1, 2, 3, 4, 5)


def ref_class(ref):
    spec = importlib.util.spec_from_file_location("ref_common_utils", os.path.join(ref, "data", "common_utils.py"))
    cu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cu)
    ns = {"torch": torch, "np": np, "glob": glob, "random": random, "os": os, "json": json, "X_PAD": 0, "Y_PAD": -1,
          "parse_csv_to_list": cu.parse_csv_to_list, "extract_timestamp": cu.extract_timestamp}
    path = os.path.join(ref, "data", "youtube_subtitle_dataset.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    # the module's own X_PAD / Y_PAD assignments, if it makes them at top level, override the defaults above
    consts = [n for n in tree.body if isinstance(n, ast.Assign) and all(
        isinstance(t, ast.Name) and t.id in ("X_PAD", "Y_PAD") for t in n.targets)]
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == NAME]
    assert len(nodes) == 1
    exec(compile(ast.Module(body=consts + nodes, type_ignores=[]), path, "exec"), ns)
    return ns[NAME], ns["X_PAD"], ns["Y_PAD"]


def main():
    import corpus_util as cu
    from data.synthetic_dataset import HashGPTTokenizer
    cls, x_pad, y_pad = ref_class(sys.argv[1])
    tok = HashGPTTokenizer()
    out = {"source": f"reference data/youtube_subtitle_dataset.py {NAME} (ast-extracted, unmodified) with model_type "
                     "'gpt' run on tests/corpus_util.py's write_corpus(hw=8) with "
                     "data.synthetic_dataset.HashGPTTokenizer()", "x_pad": x_pad, "y_pad": y_pad, "configs": []}
    with tempfile.TemporaryDirectory() as root:
        _, data_file, vid_file, _, _, _ = cu.write_corpus(root, hw=8)
        for T, L in CONFIGS:
            ds = cls(data_file, vid_file, "gpt", tok, clip_frame_num=T, max_text_len=L)
            items = []
            for seed in SEEDS:
                for i in range(len(ds.vids)):
                    random.seed(seed)
                    x, y, m = ds[i]
                    items.append({"seed": seed, "i": i, "x": x.tolist(), "y": y.tolist(), "mask": m.tolist()})
            out["configs"].append({"clip_frame_num": T, "max_text_len": L, "items": items})
    path = os.path.join(REPO, "tests", "golden", "gpt_dataset.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print("wrote", path, [len(c["items"]) for c in out["configs"]])


if __name__ == "__main__":
    main()
