"""libriichi.stat (reference libriichi/src/stat.rs): `Stat.from_dir(dir, player_name, disable_progress_bar=False)`,
`Stat.from_log`, 44 counters, derived-rate getters, `total_pt` / `avg_pt` — see mortal_amd/stat.py.  Extensions: `STAT_FIELDS`,
`Stat.from_counters` / `counters`, and `stat_logs`, the same counters computed on the device from packed event words."""
from mortal_amd.stat import STAT_FIELDS, Stat, stat_logs  # noqa: F401

__all__ = ["Stat", "STAT_FIELDS", "stat_logs"]
