"""Drop-in for reference data/youtube_chapter_title_dataset.py:23-158 (YoutubeChapterTitleDataset), the dataset
train_chapter_title_gen.py fine-tunes Pegasus on: one randomly chosen chapter per video.

Item i (tests/golden/title_dataset.json holds the reference class's own items):
  * a chapter of video i is drawn with `random.randint`; its title is the chapter line without its time stamps,
    clean_str'd, remove_timestamp'd and lower-cased; the chapter runs to the next chapter's start, the last one to
    round(duration - 1);
  * the source text is the subtitles whose start lies strictly within 1 s of the chapter (start - 1 < t < end + 1),
    joined by blanks and lower-cased, tokenised, cropped to max_text_len and padded with the pad token under mask 0 (a
    chapter without subtitles: an all-zero mask);
  * decoder input [pad] + title and targets title + [eos], both cropped to chapter_title_text_len -- a title of at least
    that many tokens has the EOS forced into the last target slot -- and padded with EOS under mask 0.
Returns (text_ids, attention_mask, input_decode_ids, decode_attention_mask, target_decode_ids), int64.

`tokenizer`: pad_token, eos_token, tokenize(text), convert_tokens_to_ids(tokens) -- transformers.PegasusTokenizer, or
data.synthetic_dataset.HashPegasusTokenizer where its files are absent. The reference module's vision-embedding and
predicted-cut-point variants, and its plotting / image imports, are not ported.
"""
import glob
import json
import os
import random

import torch

from .common_utils import clean_str, extract_first_timestamp, parse_csv_to_list, remove_timestamp

TIME_GAP = 1  # seconds of subtitles taken beyond either end of the chapter


def _pad(seq, n, fill):
    return seq + [fill] * (n - len(seq))


class YoutubeChapterTitleDataset:
    def __init__(self, data_file, vid_file, tokenizer, max_text_len=512, chapter_title_text_len=30, transform=None,
                 target_transform=None, subtitle_dir=None):
        self.tokenizer = tokenizer
        self.max_text_len = max_text_len
        self.chapter_title_text_len = chapter_title_text_len
        vids, titles, durations, timestamps = parse_csv_to_list(data_file)
        self.vid2title = dict(zip(vids, titles))
        self.vid2timestamps = dict(zip(vids, timestamps))
        self.vid2durations = dict(zip(vids, durations))
        with open(vid_file) as f:
            self.vids = [line.strip() for line in f.readlines()]
        root = os.path.dirname(data_file) if subtitle_dir is None else subtitle_dir
        self.vid2asr_files = {os.path.basename(p).split(".")[0][len("subtitle_"):]: p
                              for p in glob.glob(root + "/*/subtitle_*.json")}
        self.transform = transform
        self.target_transform = target_transform

    def __len__(self):
        return len(self.vids)

    def chapter(self, vid, k):
        """(title, source text) of chapter k of a video"""
        starts, lines = zip(*[extract_first_timestamp(line) for line in self.vid2timestamps[vid]])
        title = remove_timestamp(clean_str(lines[k])).lower()
        t0 = starts[k]
        t1 = starts[k + 1] if k + 1 < len(starts) else round(self.vid2durations[vid] - 1)
        with open(self.vid2asr_files[vid]) as f:
            subtitle = json.load(f)
        texts = []
        for sub in subtitle:
            if t0 - TIME_GAP < sub["start"] < t1 + TIME_GAP:
                texts.append(sub["text"])
            if sub["start"] >= t1 + TIME_GAP:
                break
        # (the reference starts from "" and appends with a blank only once the text is not empty: leading empty
        # subtitle texts leave no blank behind)
        text = ""
        for t in texts:
            text = t if text == "" else text + " " + t
        return title, text.lower()

    def __getitem__(self, i):
        vid = self.vids[i]
        k = random.randint(0, len(self.vid2timestamps[vid]) - 1)
        title, text = self.chapter(vid, k)
        tok, L, T = self.tokenizer, self.max_text_len, self.chapter_title_text_len
        pad, eos = tok.pad_token, tok.eos_token

        src = tok.tokenize(text)[:L]
        mask = _pad([1] * len(src), L, 0)
        src = _pad(src, L, pad)

        words = tok.tokenize(title)
        dec_in = ([pad] + words)[:T]  # the pad token is Pegasus' decoder start token
        n = min(len(words) + 1, T)
        target = (words[:T - 1] + [eos]) if len(words) >= T else words + [eos]
        dec_mask = _pad([1] * n, T, 0)
        dec_in, target = _pad(dec_in, T, eos), _pad(target, T, eos)

        ids = lambda tokens: torch.tensor(tok.convert_tokens_to_ids(tokens), dtype=torch.int64)  # noqa: E731
        return ids(src), torch.tensor(mask, dtype=torch.int64), ids(dec_in), torch.tensor(dec_mask, dtype=torch.int64), \
            ids(target)
