"""JSON training configuration -- same schema, defaults and override rules as the reference's
``dquartic/utils/config_loader.py`` (:4-57 load with CLI overrides, :60-119 default-config writer).
Additions (all optional, defaulting to the reference behaviour): ``data.synthetic`` = {"n_windows", "RT", "MZ"} selects the
built-in synthetic dataset instead of files; integer-like CLI overrides that arrive as strings (``--batch-size``,
``--threads`` have no click type in the reference, cli.py:39,42) are coerced to int; ``data.validation`` (absent from the default
config) describes a held-out set with the keys of ``data`` itself -- see ``validation_config``; ``data.mixture`` (absent from the
default config too) asks for K-component mixtures with drawn weights -- see ``mixture_config``; ``model.pred_type`` is checked against
``PRED_TYPES`` when a config is loaded (the reference's ``"eps"`` and ``"x0"``, and ``"v_prediction"``)."""
import copy
import json

DEFAULT_CONFIG = {
    "data": {"parquet_directory": "data/", "ms2_data_path": None, "ms1_data_path": None, "normalize": "minmax"},
    "model": {
        "checkpoint_path": "best_model.ckpt", "num_epochs": 10000, "warmup_epochs": 5, "batch_size": 1,
        "learning_rate": 0.00001, "num_timesteps": 1000, "beta_schedule_type": "cosine", "pred_type": "eps",
        "auto_normalize": True, "ms1_loss_weight": 0.0, "use_model": "UNet1d",
        "CustomTransformer": {"input_dim": 40000, "hidden_dim": 1024, "num_heads": 8, "num_layers": 8},
        "UNet1d": {"dim": 4, "channels": 1, "dim_mults": [1, 2, 2, 3, 3, 4, 4], "conditional": True, "init_cond_channels": 1,
                   "attn_cond_channels": 1, "tfer_dim_mult": 620, "downsample_dim": 40000, "simple": True},
    },
    "wandb": {"use_wandb": True, "wandb_project": "dquartic", "wandb_name": None, "wandb_id": None, "wandb_resume": None,
              "wandb_architecture": "DDIM(UNet1d)", "wandb_dataset": "MS2", "wandb_mode": "offline"},
    "threads": 4,
}

PRED_TYPES = ("eps", "x0", "v_prediction")  # model.pred_type: the reference's two objectives and v-prediction

_OVERRIDES = {  # kwarg -> (section, key, coerce)
    "parquet_directory": ("data", "parquet_directory", None),
    "ms2_data_path": ("data", "ms2_data_path", None),
    "ms1_data_path": ("data", "ms1_data_path", None),
    "batch_size": ("model", "batch_size", int),
    "checkpoint_path": ("model", "checkpoint_path", None),
    "use_wandb": ("wandb", "use_wandb", None),
    "threads": (None, "threads", int),
}


def load_train_config(config_path: str, **kwargs):
    with open(config_path, "r") as f:
        cfg = json.load(f)
    for key in ("parquet_directory", "ms2_data_path", "ms1_data_path"):
        cfg["data"].setdefault(key, None)
    for name, (section, key, coerce) in _OVERRIDES.items():
        val = kwargs.get(name)
        if val is None:
            continue
        if coerce is not None:
            val = coerce(val)
        if section is None:
            cfg[key] = val
        else:
            cfg[section][key] = val
    cfg["model"]["batch_size"] = int(cfg["model"]["batch_size"])
    cfg["threads"] = int(cfg.get("threads", 0))
    pred_type = cfg["model"].get("pred_type", "eps")
    if pred_type not in PRED_TYPES:
        raise ValueError(f"model.pred_type: Unknown pred_type {pred_type!r} (one of {list(PRED_TYPES)})")
    return cfg


MIXTURE_DEFAULTS = {"n_components": [2, 4], "max_ratio_log2": 3, "seed": 0, "scale_target": True}


def mixture_config(block, where="data.mixture", defaults=None):
    """A ``mixture`` block -- ``data.mixture`` or ``data.validation.mixture`` -- completed and checked, or None for an absent one (None,
    the pair at (0.5, 0.5) of the reference): the arguments of ``ResidentMixLoader``.  ``n_components`` = [kmin,
    kmax] with 1 <= kmin <= kmax and 2 <= kmax <= 8, ``max_ratio_log2`` an integer in 0..16, ``seed`` an integer, ``scale_target`` a
    boolean; a key left out takes ``defaults`` (``MIXTURE_DEFAULTS`` unless given).  Unknown keys and values out of range raise."""
    if block is None:
        return None
    if not isinstance(block, dict):
        raise ValueError(f"{where} must be an object with the keys {list(MIXTURE_DEFAULTS)}")
    unknown = sorted(set(block) - set(MIXTURE_DEFAULTS))
    if unknown:
        raise ValueError(f"{where}: unknown key(s) {unknown}; it takes {list(MIXTURE_DEFAULTS)}")
    out = {**copy.deepcopy(MIXTURE_DEFAULTS if defaults is None else defaults), **copy.deepcopy(block)}
    is_int = lambda v: isinstance(v, int) and not isinstance(v, bool)
    nc = out["n_components"]
    if not (isinstance(nc, (list, tuple)) and len(nc) == 2 and all(is_int(v) for v in nc) and 1 <= nc[0] <= nc[1] and 2 <= nc[1] <= 8):
        raise ValueError(f"{where}.n_components must be [kmin, kmax] with 1 <= kmin <= kmax and 2 <= kmax <= 8, got {nc!r}")
    out["n_components"] = [int(nc[0]), int(nc[1])]
    if not (is_int(out["max_ratio_log2"]) and 0 <= out["max_ratio_log2"] <= 16):
        raise ValueError(f"{where}.max_ratio_log2 must be an integer in 0..16, got {out['max_ratio_log2']!r}")
    if not is_int(out["seed"]):
        raise ValueError(f"{where}.seed must be an integer, got {out['seed']!r}")
    if not isinstance(out["scale_target"], bool):
        raise ValueError(f"{where}.scale_target must be true or false, got {out['scale_target']!r}")
    return out


_DATA_KEYS = ("parquet_directory", "ms2_data_path", "ms1_data_path", "normalize", "synthetic", "mixture")
_VALIDATION_ONLY_KEYS = ("n_pairs", "val_every", "seed")
VALIDATION_SYNTHETIC_START = 1_000_000  # default first window of a synthetic held-out pool: far from any training pool 0 .. n_windows-1


def validation_config(cfg):
    """The ``data.validation`` block of a loaded train config as a complete data section, or None when the config has none.  It takes
    the keys of ``data`` (``parquet_directory, ms2_data_path, ms1_data_path, normalize, synthetic``; ``normalize`` defaults to the training
    set's, the paths to None) plus ``n_pairs`` (how many index pairs of its windows form the held-out set; default: one per window),
    ``seed`` (of the generator those index pairs are drawn from; default 0 -- the set is the same in every run) and ``val_every``
    (validate after every that-many-th epoch; default 1).  A ``synthetic`` block without ``start`` gets
    ``VALIDATION_SYNTHETIC_START`` so that its windows are not the training pool's.  ``mixture`` (see ``mixture_config``) defaults to the
    training set's ``data.mixture`` with the block's ``seed``; with one, the held-out set is ``n_pairs`` K-component items.  Unknown keys
    raise."""
    val = cfg.get("data", {}).get("validation")
    if val is None:
        return None
    if not isinstance(val, dict):
        raise ValueError("data.validation must be an object with the keys of data")
    unknown = sorted(set(val) - set(_DATA_KEYS) - set(_VALIDATION_ONLY_KEYS))
    if unknown:
        raise ValueError(f"data.validation: unknown key(s) {unknown}; it takes {list(_DATA_KEYS + _VALIDATION_ONLY_KEYS)}")
    out = {"parquet_directory": None, "ms2_data_path": None, "ms1_data_path": None, "normalize": cfg["data"].get("normalize", "minmax"),
           "synthetic": None, "n_pairs": None, "val_every": 1, "seed": 0}
    out.update(copy.deepcopy(val))
    if out["synthetic"]:
        out["synthetic"].setdefault("start", VALIDATION_SYNTHETIC_START)
    elif not (out["parquet_directory"] or out["ms2_data_path"]):
        raise ValueError("data.validation needs a data source: parquet_directory / ms2_data_path + ms1_data_path, or synthetic")
    if out["n_pairs"] is not None:
        out["n_pairs"] = int(out["n_pairs"])
        if out["n_pairs"] < 1:
            raise ValueError("data.validation.n_pairs must be >= 1")
    out["seed"] = int(out["seed"])
    out["val_every"] = int(out["val_every"])
    if out["val_every"] < 1:
        raise ValueError("data.validation.val_every must be >= 1")
    # mixtures: the block's own "mixture" over the training set's values, the seed excepted -- that defaults to the block's "seed", the one
    # its items are drawn under.  Without the key the held-out set mixes what the training set mixes; an explicit null means pairs.
    train_mix = mixture_config(cfg["data"].get("mixture"))
    # The result has a "mixture" key only when one applies: a config without any mixture block gets the dict it always got.
    if "mixture" in val and val["mixture"] is None or "mixture" not in val and train_mix is None:
        out.pop("mixture", None)
    else:
        out["mixture"] = mixture_config(val.get("mixture", {}), "data.validation.mixture",
                                        {**(train_mix or MIXTURE_DEFAULTS), "seed": out["seed"]})
    return out


def generate_train_config(config_path: str):
    with open(config_path, "w") as f:
        json.dump(copy.deepcopy(DEFAULT_CONFIG), f, indent=4)
