"""Drop-in for reference data/common_utils.py (the parts on the clip-scorer path).

- `parse_csv_to_list(csv_file)` -- `common_utils.py:6-15`: the dataset CSV (columns videoId, title, duration,
  timestamp) -> (vids, titles, durations, timestamps), each video's timestamp cell split on the "%^&*" delimiter;
- `extract_timestamp`, `extract_first_timestamp` -- `common_utils.py:37-83` (restated in data/clip_windows.py);
- `clean_str`, `remove_timestamp` -- `common_utils.py:17-34, 87-109`: the chapter-title clean-up of the title dataset.
"""
import pandas as pd

from .clip_windows import extract_first_timestamp, extract_timestamp  # noqa: F401

TIMESTAMP_DELIMITER = "%^&*"


def parse_csv_to_list(csv_file):
    data = pd.read_csv(csv_file)
    vids = list(data["videoId"].values)
    titles = list(data["title"].values)
    durations = list(data["duration"].values)
    timestamps = [str(x).split(TIMESTAMP_DELIMITER) for x in data["timestamp"].values]
    return vids, titles, durations, timestamps


def write_csv(csv_file, vids, titles, durations, timestamps):
    """The inverse (test fixtures / synthetic corpora written to disk in the reference's format)."""
    pd.DataFrame({"videoId": vids, "title": titles, "duration": durations,
                  "timestamp": [TIMESTAMP_DELIMITER.join(t) for t in timestamps]}).to_csv(csv_file, index=False)


def clean_str(s):
    """The string from its first to its last alphanumeric character (chapter titles: leading / trailing punctuation
    and blanks go); a string without any is returned as it is."""
    keep = [i for i, c in enumerate(s) if c.isalnum()]
    return s[keep[0]:keep[-1] + 1] if keep else s


def remove_timestamp(s):
    """s without its first time stamp (extract_timestamp's patterns and their priority), the remaining words joined by
    single blanks; a string without a time stamp is returned as it is."""
    _, sec, si, ei = extract_timestamp(s)
    if sec == -1:
        return s
    return " ".join(w for w in (s[:si] + s[ei:]).split(" ") if w)
