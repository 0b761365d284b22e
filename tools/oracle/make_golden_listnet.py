"""Generate tests/golden/listnet_dataset.json: outputs of the REFERENCE listwise-stage dataset classes.

As tools/oracle/make_golden_contrast.py does, the script parses the reference modules with `ast` and executes only the
class definitions `YoutubeListwiseClipDataset` (data/youtube_dataset.py:1195-1388) and `InferYoutubeVideoDataset`
(data/infer_youtube_video_dataset.py:31-215) -- the reference's own code, unmodified -- in a namespace holding the real
modules they use (torch, numpy, glob, random, os, json, PIL.Image) and the reference's own `data/common_utils.py`
functions (loaded by path). Nothing is stubbed, and the reference MODEL class is never touched.

Inputs: tests/corpus_util.py's corpus writer and data.synthetic_dataset.HashTokenizer. Two configurations:
- the default corpus (40 and 57 frames) at clip_frame_num 8: 3 positive clips per video and 5 / 10 negatives, so
  negative_clip_num = 4;
- write_corpus(n_frames=(95, 120)) at clip_frame_num 8 with negative_clip_num = 10.
Python's `random` is seeded before each listwise item, as the tests do. Recorded: ids, masks, labels, and the images'
shape and digest (corpus_util.tensor_digest) -- never an image, never a path.

Usage: python tools/oracle/make_golden_listnet.py <path to the reference's video_chapter_generation directory>
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
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(REPO, "video-chapter-generation_amd"), os.path.join(REPO, "tests"), REPO):
    sys.path.insert(0, p)

LISTWISE = ("youtube_dataset.py", "YoutubeListwiseClipDataset")
INFER = ("infer_youtube_video_dataset.py", "InferYoutubeVideoDataset")
# (n_frames or None for corpus_util's default, clip_frame_num, max_text_len, negative_clip_num)
CONFIGS = [(None, 8, 24, 4), ((95, 120), 8, 50, 10)]
SEEDS = (1, 2, 3)
MODES = ("text", "all")


def ref_class(ref, file, name):
    spec = importlib.util.spec_from_file_location("ref_common_utils", os.path.join(ref, "data", "common_utils.py"))
    cu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cu)
    ns = {"torch": torch, "np": np, "glob": glob, "random": random, "os": os, "json": json, "Image": Image,
          "parse_csv_to_list": cu.parse_csv_to_list, "extract_first_timestamp": cu.extract_first_timestamp}
    path = os.path.join(ref, "data", file)
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == name]
    assert len(nodes) == 1
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns[name]


def image_record(img, digest):
    img = torch.as_tensor(img)
    return {"img_shape": list(img.shape), "img_dtype": str(img.dtype), "img_digest": digest(img)}


def main():
    import corpus_util as cu
    from data.synthetic_dataset import HashTokenizer
    from train_video_segment_point import vision_transform
    listwise, infer = ref_class(sys.argv[1], *LISTWISE), ref_class(sys.argv[1], *INFER)
    tok = HashTokenizer()
    out = {"source": "reference data/youtube_dataset.py YoutubeListwiseClipDataset and "
                     "data/infer_youtube_video_dataset.py InferYoutubeVideoDataset (ast-extracted, unmodified) run on "
                     "tests/corpus_util.py's write_corpus(hw=8) with data.synthetic_dataset.HashTokenizer; the infer "
                     "dataset's transform in mode \"all\" is train_video_segment_point.vision_transform(False)",
           "configs": []}
    for n_frames, T, L, neg in CONFIGS:
        frames = tuple(n_frames) if n_frames is not None else cu.N_FRAMES
        with tempfile.TemporaryDirectory() as root:
            img_dir, data_file, vid_file, _, _, _ = cu.write_corpus(root, n_videos=len(frames), n_frames=frames, hw=8)
            cfg = {"n_frames": list(frames), "clip_frame_num": T, "max_text_len": L, "negative_clip_num": neg,
                   "listwise": [], "infer": []}
            for mode in MODES:
                ds = listwise(img_dir, data_file, vid_file, tok, T, L, negative_clip_num=neg, mode=mode)
                for seed in SEEDS:
                    for i in range(len(ds)):
                        random.seed(seed)
                        img, ids, mask, labels = ds[i]
                        rec = {"mode": mode, "seed": seed, "i": i, "ids": ids.tolist(), "mask": mask.tolist(),
                               "labels": labels.tolist()}
                        rec.update(image_record(img, cu.tensor_digest))
                        cfg["listwise"].append(rec)
                dv = infer(img_dir, data_file, vid_file, tok, T, L, mode=mode, transform=vision_transform(False))
                for vid in dv.vids:
                    dv.manual_choose_vid(vid)
                    items = []
                    for i in range(len(dv)):
                        img, ids, mask, label = dv[i]
                        rec = {"ids": ids.tolist(), "mask": mask.tolist(), "label": int(label)}
                        rec.update(image_record(img, cu.tensor_digest))
                        items.append(rec)
                    cfg["infer"].append({"mode": mode, "vid": vid, "duration": dv.get_duration(), "items": items})
            out["configs"].append(cfg)
    path = os.path.join(REPO, "tests", "golden", "listnet_dataset.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print("wrote", path, os.path.getsize(path), "bytes",
          [(len(c["listwise"]), sum(len(v["items"]) for v in c["infer"])) for c in out["configs"]])


if __name__ == "__main__":
    main()
