"""Generate tests/golden/title_dataset.json: items of the REFERENCE class YoutubeChapterTitleDataset.

As tools/oracle/make_golden_gpt.py does, the script parses the reference module `data/youtube_chapter_title_dataset.py`
with `ast` and executes only the class definition `YoutubeChapterTitleDataset` (:23-158) -- the reference's own code,
unmodified -- in a namespace holding the real modules it uses (torch, numpy, glob, random, os, json) and the
reference's own `data/common_utils.py` functions (loaded by path). The reference is read at run time only; nothing of
it is written anywhere but the recorded items.

Inputs: tests/title_corpus_util.py's corpus (tests/corpus_util.py's two videos with one chapter's subtitles removed)
and data.synthetic_dataset.HashPegasusTokenizer(515). Python's `random` is seeded before each item, as the tests do.
The configs crop the source (6), pad it (40) and include title lengths 2 and 3 against the 2-token titles, so a title
of at least chapter_title_text_len tokens is recorded; the script checks that and that the chapter without subtitles
(an all-zero source mask) was drawn.

Usage: python tools/oracle/make_golden_title.py <path to the reference's video_chapter_generation directory>
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

NAME = "YoutubeChapterTitleDataset"


def ref_class(ref):
    spec = importlib.util.spec_from_file_location("ref_common_utils", os.path.join(ref, "data", "common_utils.py"))
    cu = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cu)
    ns = {"torch": torch, "np": np, "glob": glob, "random": random, "os": os, "json": json,
          "parse_csv_to_list": cu.parse_csv_to_list, "extract_first_timestamp": cu.extract_first_timestamp,
          "remove_timestamp": cu.remove_timestamp, "clean_str": cu.clean_str}
    path = os.path.join(ref, "data", "youtube_chapter_title_dataset.py")
    with open(path) as f:
        tree = ast.parse(f.read(), filename=path)
    nodes = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == NAME]
    assert len(nodes) == 1
    exec(compile(ast.Module(body=nodes, type_ignores=[]), path, "exec"), ns)
    return ns[NAME]


def main():
    import title_corpus_util as tc
    from data.synthetic_dataset import HashPegasusTokenizer
    cls = ref_class(sys.argv[1])
    tok = HashPegasusTokenizer(tc.VOCAB)
    out = {"source": f"reference data/youtube_chapter_title_dataset.py {NAME} (ast-extracted, unmodified) run on "
                     "tests/title_corpus_util.py's write_title_corpus with "
                     f"data.synthetic_dataset.HashPegasusTokenizer({tc.VOCAB})", "configs": []}
    names = ("text_ids", "attention_mask", "input_decode_ids", "decode_attention_mask", "target_decode_ids")
    empty = long_title = False
    with tempfile.TemporaryDirectory() as root:
        data_file, vid_file = tc.write_title_corpus(root)
        for L, T in tc.CONFIGS:
            ds = cls(data_file, vid_file, tok, max_text_len=L, chapter_title_text_len=T)
            items = []
            for seed in tc.SEEDS:
                for i in range(len(ds)):
                    random.seed(seed)
                    item = ds[i]
                    items.append(dict({"seed": seed, "i": i}, **{n: t.tolist() for n, t in zip(names, item)}))
                    empty |= int(item[1].sum()) == 0
                    long_title |= int(item[3].sum()) == T and int(item[4][-1]) == 1 and T <= 2
            out["configs"].append({"max_text_len": L, "chapter_title_text_len": T, "items": items})
    assert empty and long_title, (empty, long_title)
    path = os.path.join(REPO, "tests", "golden", "title_dataset.json")
    with open(path, "w") as f:
        json.dump(out, f)
    print("wrote", path, [len(c["items"]) for c in out["configs"]])


if __name__ == "__main__":
    main()
