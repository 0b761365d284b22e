"""The corpus of the title-dataset golden (test helper; also used by tools/oracle/make_golden_title.py):
tests/corpus_util.py's two videos, with the subtitles of the second video's chapter 1 (9 s to 21 s, with the dataset's
1 s margin: 8 < start < 22) removed, so that one chapter has no subtitles at all."""
import json
import os

import corpus_util as cu

EMPTY_VIDEO, EMPTY_CHAPTER, EMPTY_SPAN = 1, 1, (8.0, 22.0)
CONFIGS = [(40, 30), (6, 2), (16, 3)]  # (max_text_len, chapter_title_text_len); titles are "part k": 2 tokens
SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
VOCAB = 515


def write_title_corpus(root):
    """-> (data_file, vid_file)"""
    _, data_file, vid_file, subs, _, _ = cu.write_corpus(root, hw=8)
    vid = cu.VIDS[EMPTY_VIDEO]
    kept = [s for s in subs[vid] if not EMPTY_SPAN[0] < s["start"] < EMPTY_SPAN[1]]
    with open(os.path.join(root, "subs", vid, f"subtitle_{vid}.json"), "w") as f:
        json.dump(kept, f)
    return data_file, vid_file
