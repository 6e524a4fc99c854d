"""evals.datasets.taskonomy — the reference's per-sample wrapper (evals/datasets/taskonomy.py:62-84): an indexable dataset of decoded
samples {"rgb", <task>, "mask_valid", ...} -> {"rgb": float32 [3, H, W] ImageNet-normalised, <task>: float32 [Ct, H, W], "mask_valid":
bool [1, H, W]}, every other key dropped.  ``task == "depth"`` reads and returns the key "depth" with depth_euclidean's transform."""
from __future__ import annotations

import torch

from .transforms import task_transform


def Taskonomy(*args, **kwargs):
    """The reference's reader (taskonomy.py:31-59) loads two Hugging Face ``datasets`` repositories; that package and the network are
    not part of this path."""
    raise NotImplementedError("Taskonomy(): the Hugging Face `datasets` reader is out of scope; wrap any indexable dataset of decoded "
                              "samples in TaskonomyDataset(dataset, task), or use evals.datasets.synthetic.SyntheticTaskonomy")


class TaskonomyDataset(torch.utils.data.Dataset):
    def __init__(self, dataset, task):
        from mvp.taskonomy import resolve_task

        resolve_task("depth_euclidean" if task == "depth" else task)  # out-of-scope tasks fail here, not at the first sample
        self.dataset = dataset
        self.task = task

    def __getitem__(self, idx):
        item = self.dataset[idx]
        task = "depth_euclidean" if self.task == "depth" else self.task
        return {"rgb": task_transform(item["rgb"], "rgb"), self.task: task_transform(item[self.task], task),
                "mask_valid": task_transform(item["mask_valid"], "mask_valid")}

    def __len__(self):
        return len(self.dataset)
