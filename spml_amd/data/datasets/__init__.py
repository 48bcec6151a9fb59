from spml_amd.data.datasets.base_dataset import ListDataset  # noqa: F401
from spml_amd.data.datasets.densepose_dataset import DenseposeClassifierDataset, DenseposeDataset  # noqa: F401
from spml_amd.data.datasets.list_tag_dataset import ListTagClassifierDataset, ListTagDataset  # noqa: F401
