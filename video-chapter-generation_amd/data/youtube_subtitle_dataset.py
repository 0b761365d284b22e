"""Drop-in for reference data/youtube_subtitle_dataset.py `YoutubeClipSubtitleDatasetForHugFace` (:248-408), the
masked-LM pre-training sampler of pretrain_lang_model_hugface.py: same constructor, same sample tuple, same rules.

    YoutubeClipSubtitleDatasetForHugFace(data_file, vid_file, model_type, tokenizer, clip_frame_num, max_text_len,
                                         subtitle_dir=None, transform=None, target_transform=None)
    item i -> (text_ids i64 [L], targets i64 [L] (-1 = not masked), attention_mask i64 [L])

- item i draws one clip centre t of video i with Python `random` from [T/2, image_num - T/2), image_num =
  round(duration - 1) (:293, :309-314);
- the text is every subtitle starting inside (t - T/2 - 4, t + T/2 + 4), joined by spaces (:317-326);
- `bert` branch (:349-402): "[CLS] " + text, tokenised, truncated to max_text_len, masked by `mask_tokens`, padded
  with "[PAD]" (attention mask 0), converted to ids; the targets are the original ids at the masked positions;
- `gpt` (next-token targets, :329-347) is not a branch of this class: the constructor raises. The generative stage
  has a class of its own, `YoutubeClipSubtitleDatasetForGPT` (below), next to the contrastive stage's.

`SyntheticSubtitleDatasetForHugFace` runs the same sampler over data/synthetic_dataset.py's corpus, so the driver runs
with no data on disk.

`YoutubeClipSubtitleDatasetForGPT(data_file, vid_file, tokenizer, clip_frame_num, max_text_len, subtitle_dir=None)` is
the reference class's `gpt` branch (:329-347) over the same clip sampler: ids = tokenizer(text).data["input_ids"],
x = ids[:-1], y = ids[1:], both truncated to max_text_len and padded with X_PAD / Y_PAD; the attention mask is 1 over
len(y). item i -> (x i64 [L], y i64 [L] (-1 = padding), attention_mask i64 [L]). `SyntheticSubtitleDatasetForGPT` is
its synthetic-corpus twin.

`YoutubeClipConstrastSubtitleDataset` (:415-551) is the shot-contrastive sampler of
train_lang/pretrain_constrast_lang_model.py:

    YoutubeClipConstrastSubtitleDataset(data_file, vid_file, tokenizer, clip_frame_num, max_text_len, neighbor_size=3,
                                        transform=None, target_transform=None, subtitle_dir=None)
    item i -> (query ids i64 [L], query mask [L], candidate ids [2 n, L], candidate masks [2 n, L])

- item i draws the query clip's start t of video i from [n T, duration - (n + 1) T), duration = round(duration - 1)
  (:458-471); the 2 n + 1 clips are the n clips of T seconds before it, the query and the n after it;
- each clip's text is its subtitles joined by spaces, "[CLS] " in front, truncated and padded as above, unmasked;
- a video too short for the neighbours, or a clip without any subtitle, makes the reference draw another video with
  random.randint and start over (:468-470, :508-510); so does this class, draw for draw.
`SyntheticClipConstrastSubtitleDataset` is its synthetic-corpus twin.
"""
import json
import os
import random

import numpy as np
import torch

from .common_utils import parse_csv_to_list
from .youtube_dataset import subtitle_files

X_PAD = 0
Y_PAD = -1
TEXT_EXTRA_TIME_GAP = 4


def mask_tokens(tokens, rng):
    """The masking rule of :356-380 on a token list whose position 0 ([CLS]) is never masked; `rng` is the `random`
    module or a random.Random, consumed call for call as the reference consumes `random`. Returns (the masked token
    list, {position: original token}).

    round(n * 0.15) of the n = len(tokens) - 1 maskable positions are drawn (Python's round: n <= 3 gives none) and
    set to "[MASK]"; 10 % of those are then drawn to stay unmasked and 10 % to be replaced. Two quirks are kept:
    the reference's "restore" loop assigns each such token to itself, so the positions drawn to stay unmasked stay
    "[MASK]" (the draw still advances the generator); and each replacement is sampled from the token list as it
    stands after masking, "[MASK]" and "[CLS]" included."""
    tokens = list(tokens)
    positions = list(range(1, len(tokens)))
    masked = rng.sample(positions, round(len(positions) * 0.15))
    rng.sample(masked, round(len(masked) * 0.1))  # the "not masked" draw: without effect, see above
    replaced = rng.sample(masked, round(len(masked) * 0.1))
    original = {}
    for pos in masked:
        original[pos] = tokens[pos]
        tokens[pos] = "[MASK]"
    for pos in replaced:
        tokens[pos] = rng.sample(tokens, 1)[0]
    return tokens, original


def clip_text(subtitles, t, half_clip_frame_num):
    """Subtitles starting strictly inside (clip start - 4 s, clip end + 4 s) of the clip centred at t (:313-326)."""
    lo = t - half_clip_frame_num - TEXT_EXTRA_TIME_GAP
    hi = t + half_clip_frame_num + TEXT_EXTRA_TIME_GAP
    text = ""
    for sub in subtitles:
        if lo < sub["start"] < hi:
            text = text + " " + sub["text"] if text else sub["text"]  # (no separator while the text is still empty)
    return text


def encode_mlm(tokenizer, text, max_text_len, rng):
    """:349-402 -> (ids, targets, attention_mask) as int64 tensors of max_text_len."""
    tokens = tokenizer.tokenize("[CLS] " + text)[:max_text_len]
    tokens, original = mask_tokens(tokens, rng)
    n_pad = max(0, max_text_len - len(tokens))
    mask = [1] * len(tokens) + [0] * n_pad
    tokens = tokens + ["[PAD]"] * n_pad
    ids = tokenizer.convert_tokens_to_ids(tokens)
    y = [Y_PAD] * len(tokens)
    for pos, tok in original.items():
        y[pos] = tokenizer.convert_tokens_to_ids([tok])[0]
    return tuple(torch.from_numpy(np.array(a)).long() for a in (ids, y, mask))


def _check_model_type(model_type):
    if model_type != "bert":
        raise RuntimeError(f"model_type {model_type!r}: only the reference's 'bert' (masked-LM) branch is built here")


class YoutubeClipSubtitleDatasetForHugFace(torch.utils.data.Dataset):
    def __init__(self, data_file, vid_file, model_type, tokenizer, clip_frame_num, max_text_len, subtitle_dir=None,
                 transform=None, target_transform=None):
        _check_model_type(model_type)
        self.model_type = model_type
        self.tokenizer = tokenizer
        self.clip_frame_num = clip_frame_num
        self.half_clip_frame_num = int(clip_frame_num // 2)
        self.max_text_len = max_text_len
        vids, titles, durations, timestamps = parse_csv_to_list(data_file)
        self.vid2title = dict(zip(vids, titles))
        self.vid2timestamps = dict(zip(vids, timestamps))
        self.vid2durations = dict(zip(vids, durations))
        with open(vid_file) as f:
            self.vids = [x.strip() for x in f.readlines()]
        self.vid2asr_files = subtitle_files(os.path.dirname(data_file) if subtitle_dir is None else subtitle_dir)
        self.transform = transform
        self.target_transform = target_transform

    def __len__(self):
        return len(self.vids)

    def __getitem__(self, i):
        vid = self.vids[i]
        image_num = round(self.vid2durations[vid] - 1)
        with open(self.vid2asr_files[vid]) as f:
            subtitles = json.load(f)
        h = self.half_clip_frame_num
        t = random.sample(list(range(h, image_num - h)), k=1)[0]
        return encode_mlm(self.tokenizer, clip_text(subtitles, t, h), self.max_text_len, random)


def encode_gpt(tokenizer, text, max_text_len, vocab_size=None):
    """:329-347 -> (x, y, attention_mask) as int64 tensors of max_text_len: next-token pairs of the tokenised text.
    vocab_size: an id outside [0, vocab_size) is a ValueError here, on the host (the model's embedding kernels index
    the table by id and do not check)."""
    ids = list(tokenizer(text).data["input_ids"])
    if vocab_size is not None and ids and not (0 <= min(ids) and max(ids) < vocab_size):
        raise ValueError(f"encode_gpt: token id outside [0, {vocab_size}) (a tokenizer with another vocabulary?)")
    x = ids[:-1][:max_text_len]
    y = ids[1:][:max_text_len]
    mask = [1] * len(y)
    n_pad = max(0, max_text_len - len(x))
    x = x + [X_PAD] * n_pad
    y = y + [Y_PAD] * n_pad
    mask = mask + [X_PAD] * n_pad
    return tuple(torch.from_numpy(np.array(a, dtype=np.int64)).long() for a in (x, y, mask))


class YoutubeClipSubtitleDatasetForGPT(YoutubeClipSubtitleDatasetForHugFace):
    """The reference class with model_type "gpt" (:329-347): the masked-LM class's clip sampler, next-token targets."""

    def __init__(self, data_file, vid_file, tokenizer, clip_frame_num, max_text_len, subtitle_dir=None,
                 vocab_size=None):
        super().__init__(data_file, vid_file, "bert", tokenizer, clip_frame_num, max_text_len, subtitle_dir)
        self.model_type = "gpt"
        self.vocab_size = vocab_size  # (optional: ids are checked against it, see encode_gpt)

    def __getitem__(self, i):
        vid = self.vids[i]
        image_num = round(self.vid2durations[vid] - 1)
        with open(self.vid2asr_files[vid]) as f:
            subtitles = json.load(f)
        h = self.half_clip_frame_num
        t = random.sample(list(range(h, image_num - h)), k=1)[0]
        return encode_gpt(self.tokenizer, clip_text(subtitles, t, h), self.max_text_len, self.vocab_size)


class SyntheticSubtitleDatasetForGPT(torch.utils.data.Dataset):
    """The same sampler over a data.synthetic_dataset.SyntheticVideoCorpus (image_num frames at 1 fps)."""

    def __init__(self, corpus, tokenizer, clip_frame_num, max_text_len, vocab_size=None):
        self.c, self.tokenizer, self.max_text_len, self.vocab_size = corpus, tokenizer, max_text_len, vocab_size
        self.half_clip_frame_num = int(clip_frame_num // 2)

    def __len__(self):
        return len(self.c.vids)

    def __getitem__(self, i):
        vid = self.c.vids[i]
        h = self.half_clip_frame_num
        t = random.sample(list(range(h, self.c.image_num[vid] - h)), k=1)[0]
        return encode_gpt(self.tokenizer, clip_text(self.c.subtitles[vid], t, h), self.max_text_len, self.vocab_size)


def contrast_clips(t, clip_frame_num, neighbor_size):
    """[start, end] seconds of the 2 n + 1 clips around the query clip starting at t, in time order: n left
    neighbours, the query, n right neighbours (:473-485)."""
    T, n = clip_frame_num, neighbor_size
    return [[t + (j - n) * T, t + (j - n + 1) * T] for j in range(2 * n + 1)]


def contrast_clip_texts(subtitles, clips):
    """{clip index: its subtitles joined by spaces} by the reference's single pass (:488-504): the clip index advances
    by at most one per subtitle, when the subtitle starts after the current clip's end, and a subtitle belongs to the
    current clip if it starts inside [start, end], both ends included."""
    texts, ci = {}, 0
    for sub in subtitles:
        start = sub["start"]
        if start > clips[ci][1]:
            ci += 1
        if ci >= len(clips):
            break
        s, e = clips[ci]
        if s <= start <= e:
            texts[ci] = texts[ci] + " " + sub["text"] if ci in texts else sub["text"]
    return texts


def encode_plain(tokenizer, text, max_text_len):
    """:514-535 -> (ids, attention_mask) int64 [max_text_len]: "[CLS] " + text, truncated, padded with "[PAD]"."""
    tokens = tokenizer.tokenize("[CLS] " + text)[:max_text_len]
    n_pad = max(0, max_text_len - len(tokens))
    mask = [1] * len(tokens) + [0] * n_pad
    ids = tokenizer.convert_tokens_to_ids(tokens + ["[PAD]"] * n_pad)
    return torch.from_numpy(np.array(ids)).long(), torch.from_numpy(np.array(mask)).long()


def contrast_item(subtitles, duration, tokenizer, clip_frame_num, max_text_len, neighbor_size, rng):
    """One sample of the shot-contrastive sampler (:463-547) from a video of `duration` seconds, or None where the
    reference draws another video: the video is too short for n neighbours on each side (:468-470, before any draw),
    or one of the 2 n + 1 clips has no subtitle (:508-510, after the clip draw). `rng` is the `random` module or a
    random.Random, consumed call for call.

    -> (query ids [L], query mask [L], candidate ids [2 n, L], candidate masks [2 n, L]); the candidates are the left
    neighbours in time order, then the right ones."""
    n = neighbor_size
    t_candidate = list(range(n * clip_frame_num, duration - (n + 1) * clip_frame_num))
    if len(t_candidate) <= 0:
        return None
    t = rng.sample(t_candidate, k=1)[0]
    texts = contrast_clip_texts(subtitles, contrast_clips(t, clip_frame_num, n))
    if len(texts) < 2 * n + 1:
        return None
    enc = [encode_plain(tokenizer, texts[j], max_text_len) for j in range(2 * n + 1)]
    ids, masks = [e[0] for e in enc], [e[1] for e in enc]
    return (ids[n], masks[n], torch.stack(ids[:n] + ids[n + 1:], dim=0), torch.stack(masks[:n] + masks[n + 1:], dim=0))


class YoutubeClipConstrastSubtitleDataset(torch.utils.data.Dataset):
    """Drop-in for the reference's `YoutubeClipConstrastSubtitleDataset` (:415-551), the sampler of
    train_lang/pretrain_constrast_lang_model.py: same constructor, same sample tuple, same draws of `random`. An item
    that cannot be built from video i is replaced by one of a video drawn with random.randint, as there."""

    def __init__(self, data_file, vid_file, tokenizer, clip_frame_num, max_text_len, neighbor_size=3, transform=None,
                 target_transform=None, subtitle_dir=None):
        self.tokenizer = tokenizer
        self.clip_frame_num = clip_frame_num
        self.half_clip_frame_num = int(clip_frame_num // 2)
        self.max_text_len = max_text_len
        self.neighbor_size = neighbor_size
        vids, titles, durations, timestamps = parse_csv_to_list(data_file)
        self.vid2title = dict(zip(vids, titles))
        self.vid2timestamps = dict(zip(vids, timestamps))
        self.vid2durations = dict(zip(vids, durations))
        with open(vid_file) as f:
            self.vids = [x.strip() for x in f.readlines()]
        self.vid2asr_files = subtitle_files(os.path.dirname(data_file) if subtitle_dir is None else subtitle_dir)
        self.transform = transform
        self.target_transform = target_transform

    def __len__(self):
        return len(self.vids)

    def __getitem__(self, i):
        while True:
            vid = self.vids[i]
            duration = round(self.vid2durations[vid] - 1)
            with open(self.vid2asr_files[vid]) as f:
                subtitles = json.load(f)
            item = contrast_item(subtitles, duration, self.tokenizer, self.clip_frame_num, self.max_text_len,
                                 self.neighbor_size, random)
            if item is not None:
                return item
            i = random.randint(0, len(self.vids) - 1)


class SyntheticClipConstrastSubtitleDataset(torch.utils.data.Dataset):
    """The same sampler over a data.synthetic_dataset.SyntheticVideoCorpus (image_num seconds at 1 fps). A corpus
    without any video long enough for the neighbours is refused (the re-draw would never end)."""

    def __init__(self, corpus, tokenizer, clip_frame_num, max_text_len, neighbor_size=3):
        self.c, self.tokenizer = corpus, tokenizer
        self.clip_frame_num, self.max_text_len, self.neighbor_size = clip_frame_num, max_text_len, neighbor_size
        need = (2 * neighbor_size + 1) * clip_frame_num
        if not any(corpus.image_num[v] > need for v in corpus.vids):
            raise ValueError(f"SyntheticClipConstrastSubtitleDataset: no video longer than {need} s "
                             f"({2 * neighbor_size + 1} clips of {clip_frame_num} s)")

    def __len__(self):
        return len(self.c.vids)

    def __getitem__(self, i):
        while True:
            vid = self.c.vids[i]
            item = contrast_item(self.c.subtitles[vid], self.c.image_num[vid], self.tokenizer, self.clip_frame_num,
                                 self.max_text_len, self.neighbor_size, random)
            if item is not None:
                return item
            i = random.randint(0, len(self.c.vids) - 1)


class SyntheticSubtitleDatasetForHugFace(torch.utils.data.Dataset):
    """The same sampler over a data.synthetic_dataset.SyntheticVideoCorpus (image_num frames at 1 fps)."""

    def __init__(self, corpus, model_type, tokenizer, clip_frame_num, max_text_len):
        _check_model_type(model_type)
        self.c, self.tokenizer, self.max_text_len = corpus, tokenizer, max_text_len
        self.half_clip_frame_num = int(clip_frame_num // 2)

    def __len__(self):
        return len(self.c.vids)

    def __getitem__(self, i):
        vid = self.c.vids[i]
        h = self.half_clip_frame_num
        t = random.sample(list(range(h, self.c.image_num[vid] - h)), k=1)[0]
        return encode_mlm(self.tokenizer, clip_text(self.c.subtitles[vid], t, h), self.max_text_len, random)
