"""File-list data loading (the reference's `spml/data`): dataset classes that decode and plan on the host, and the
batcher that makes the training batch on the GPU with one augmentation launch (csrc/augment.hip)."""
from spml_amd.data.batcher import DeviceBatcher  # noqa: F401
