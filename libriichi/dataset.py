"""libriichi.dataset (reference libriichi/src/dataset/): `GameplayLoader`, `Gameplay`, `Grp` — see mortal_amd/dataset.py.
`SampleStore` (mortal_amd/samples.py) has no reference counterpart in the crate: it is the buffer of mortal/dataloader.py kept on the device."""
from mortal_amd.dataset import GameplayLoader, Gameplay, Grp  # noqa: F401
from mortal_amd.samples import SampleStore  # noqa: F401

__all__ = ["GameplayLoader", "Gameplay", "Grp", "SampleStore"]
