"""Writes tests/golden/bbknn_kat.json: two known answers worked by hand, none of them computed.

The list.  Six points on a line at 0, 1, 3, 6, 10, 15, batches 0, 1, 0, 1, 0, 1, neighbors_within_batch = 2, so K = 3: two
points of the other batch and one other point of the own batch, ascending by (distance, index).  Point 2 (at 3) meets point 0
and point 3 at the same distance 3: the lower index comes first.

Trimming.  A symmetric 5 x 5 matrix with trim = 2.  Row 0 has three entries, its second largest is 0.5; row 2 has four
(0.5, 0.5, 0.4, 0.1), its second largest is 0.5 as well; the other rows have at most two entries and the threshold 0.  The pair
(0, 3) = 0.2 falls below row 0's threshold, (1, 2) = 0.4 and (2, 4) = 0.1 below row 2's; (0, 2) and (2, 3) sit AT a threshold
and stay.  Row 4 loses its only entry.

    python tests/golden/make_bbknn_golden.py
"""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))

LIST = {
    "points": [0, 1, 3, 6, 10, 15],
    "batch": [0, 1, 0, 1, 0, 1],
    "n_batches": 2,
    "neighbors_within_batch": 2,
    "indices": [[1, 2, 3], [0, 2, 3], [1, 0, 3], [2, 4, 1], [3, 5, 2], [4, 3, 2]],
    "distances": [[1, 3, 6], [1, 2, 5], [2, 3, 3], [3, 4, 5], [4, 5, 7], [5, 9, 12]],
}

TRIM = {
    "n": 5,
    "trim": 2,
    "entries": [[0, 1, 0.9], [0, 2, 0.5], [0, 3, 0.2], [1, 2, 0.4], [2, 3, 0.5], [2, 4, 0.1]],      # i < j; the matrix is symmetric
    "thresholds": [0.5, 0.0, 0.5, 0.0, 0.0],
    "kept": [[0, 1, 0.9], [0, 2, 0.5], [2, 3, 0.5]],
    "info": {"trim": 2, "rows_over_trim": 2, "nnz_before": 12, "nnz_after": 6, "entries_trimmed": 6, "max_row_nnz_before": 4,
             "max_row_nnz_after": 2, "rows_emptied": 1},
}

if __name__ == "__main__":
    with open(os.path.join(HERE, "bbknn_kat.json"), "w") as f:
        json.dump({"list": LIST, "trim": TRIM}, f, indent=1)
        f.write("\n")
