"""Drop-ins for reference data/infer_youtube_video_dataset.py `InferYoutubeVideoDataset` (:31-215, one chosen video's
clips from start to end: the listwise stage's test pass, see the class) and `InferYoutubeClipDataset` (:218-313): the eval
dataset over the pre-flattened clip JSON (video_chapter_youtube_dataset/flat_video2clip_for_quick_infer.py; written
here by data.clip_windows.video_clip_infos). Same constructor and sample tuple:

    InferYoutubeClipDataset(img_dir, json_paths, tokenizer, clip_frame_num, max_text_len, mode="all",
                            transform=None, target_transform=None)
    item i -> (img_clip f32 [T, 3, H, W] (0 in text mode), text_ids i64 [L], attention_mask i64 [L], clip_label)

json_paths: one JSON file or a list of them (records concatenated in order); `all_clip_infos` is the record
list the trainers write `pred_score` into. Frames are the records' `image_paths`, decoded with PIL -> RGB ->
`transform`; `u8=True` returns the u8 [T, H, W, 3] stack for the GPU ingest kernel instead.
"""
import glob
import json
import os
import random

import torch

from . import clip_windows as cw
from .common_utils import parse_csv_to_list
from .youtube_dataset import frames_tensor, subtitle_files


class InferYoutubeClipDataset(torch.utils.data.Dataset):
    def __init__(self, img_dir, json_paths, tokenizer, clip_frame_num, max_text_len, mode="all", transform=None,
                 target_transform=None, u8=False):
        self.max_offset = 2
        self.tokenizer = tokenizer
        self.clip_frame_num = clip_frame_num
        self.max_text_len = max_text_len
        self.mode = mode
        self.half_clip_frame_num = int(clip_frame_num // 2)
        self.img_dir = img_dir
        if isinstance(json_paths, (list, tuple)):
            self.all_clip_infos = []
            for p in json_paths:
                with open(p, "r", encoding="utf-8") as f:
                    self.all_clip_infos.extend(json.load(f))
        else:
            with open(json_paths) as f:
                self.all_clip_infos = json.load(f)
        self.transform = transform
        self.target_transform = target_transform
        self.u8 = u8

    def __len__(self):
        return len(self.all_clip_infos)

    def __getitem__(self, i):
        info = self.all_clip_infos[i]
        ids, mask = cw.encode_text(self.tokenizer, info["text_clip"], self.max_text_len)
        img_clip = 0 if self.mode == "text" else frames_tensor(info["image_paths"], self.transform, self.u8)
        return img_clip, torch.from_numpy(ids), torch.from_numpy(mask), info["clip_label"]


def video_clip_item(win, i, cut_points, subtitles, tokenizer, clip_frame_num, max_text_len):
    """(text_ids, attention_mask, label) of clip i of one video (reference :133-180)."""
    s, e = win[i].tolist()
    label = int(cw.clip_labels(win[i:i + 1], cut_points, clip_frame_num)[0])
    ids, mask = cw.encode_text(tokenizer, cw.window_text(subtitles, s, e), max_text_len)
    return torch.from_numpy(ids), torch.from_numpy(mask), label


class InferYoutubeVideoDataset(torch.utils.data.Dataset):
    """Reference :31-215: the clips of ONE video, every 4 s from its start, chosen first by `manual_choose_vid(vid)` or
    `random_choose_vid()`; before that `len()` and indexing raise the reference's RuntimeError.

        item i -> (img_clip f32 [T, 3, H, W] through `transform` (0 in text mode), text_ids i64 [L],
                   attention_mask i64 [L], label)

    Cut points are kept for 4 <= sec <= N - 4 (:99-107)."""

    def __init__(self, img_dir, data_file, vid_file, tokenizer, clip_frame_num, max_text_len, mode="all",
                 transform=None, target_transform=None, subtitle_dir=None):
        self.max_offset = 2
        self.tokenizer = tokenizer
        self.clip_frame_num = clip_frame_num
        self.max_text_len = max_text_len
        self.mode = mode
        self.half_clip_frame_num = int(clip_frame_num // 2)
        self.img_dir = img_dir
        vids, titles, durations, timestamps = parse_csv_to_list(data_file)
        self.vid2title = dict(zip(vids, titles))
        self.vid2timestamps = dict(zip(vids, timestamps))
        self.vid2durations = dict(zip(vids, durations))
        with open(vid_file) as f:
            self.vids = [x.strip() for x in f.readlines()]
        self.asr_files = subtitle_files(os.path.dirname(data_file) if subtitle_dir is None else subtitle_dir)
        self.infer_vid = None
        self.transform = transform
        self.target_transform = target_transform

    def manual_choose_vid(self, vid):
        if vid in self.vids:
            self.infer_vid = vid
        else:
            raise RuntimeError(f"The vid {vid} is not existed in dataset")
        self._load_gt_data()

    def random_choose_vid(self):
        self.infer_vid = random.sample(self.vids, 1)[0]
        self._load_gt_data()

    def _image_num(self):
        return len(glob.glob(os.path.join(self.img_dir, self.infer_vid) + "/*.jpg"))

    def _load_gt_data(self):
        with open(self.asr_files[self.infer_vid]) as f:
            self.subtitles = json.load(f)
        self.cut_points = cw.cut_points_from_timestamps(self.vid2timestamps[self.infer_vid], self._image_num(),
                                                        mode="eval")
        self.real_cut_points = list(self.cut_points)

    def _chosen(self):
        if self.infer_vid is None:
            raise RuntimeError("You should run choose_vid before iterate this dataset")

    def __len__(self):
        self._chosen()
        return len(cw.clip_windows(self._image_num(), self.clip_frame_num, self.max_offset))

    def get_duration(self):
        return self._image_num()

    def __getitem__(self, i):
        self._chosen()
        image_num = self._image_num()
        T = self.clip_frame_num
        win = cw.clip_windows(image_num, T, self.max_offset)
        ids, mask, label = video_clip_item(win, i, self.cut_points, self.subtitles, self.tokenizer, T,
                                           self.max_text_len)
        if self.mode == "text":
            img_clip = 0
        else:
            nums = cw.frame_numbers(int(win[i, 0]), T, image_num)
            img_clip = frames_tensor([os.path.join(self.img_dir, self.infer_vid, "%05d.jpg" % n)
                                      for n in nums.tolist()], self.transform, False)
        return img_clip, ids, mask, label
