"""libriichi.arena (reference libriichi/src/arena/mod.rs): the HIP-backed batched self-play arena."""
from mortal_amd.arena import OneVsThree, TwoVsTwo  # noqa: F401
from mortal_amd.arena import SelfPlayRunner  # noqa: F401  (an extension: self-play on a restarting pool, finished games collected on the device)
