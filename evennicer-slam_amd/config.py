"""YAML configurations in the reference's format (src/config.py): a file may name a parent with `inherit_from`; the chain
is loaded root first and every child is merged over it key by key, recursively through nested mappings.  `default_path`
is the root of a chain whose last file names no parent (the reference passes configs/nice_slam.yaml)."""
import os

import yaml


def update_recursive(base, override):
    """Merge `override` into `base` in place: mappings merge key by key, anything else replaces; keys `base` lacks are kept."""
    for key, value in override.items():
        if isinstance(value, dict) and isinstance(base.get(key), dict):
            update_recursive(base[key], value)
        elif isinstance(value, dict):
            base[key] = {}
            update_recursive(base[key], value)
        else:
            base[key] = value
    return base


def load_config(path, default_path=None):
    """The configuration dict of `path` with its `inherit_from` chain (and `default_path` under the chain's root) merged."""
    chain, seen = [], set()
    while path is not None:
        if path in seen:
            raise ValueError(f"inherit_from cycle through {path}")
        seen.add(path)
        with open(path, 'r') as f:
            special = yaml.safe_load(f) or {}
        chain.append(special)
        parent = special.get('inherit_from')
        if parent is not None and not os.path.exists(parent):       # the reference resolves against the working directory only
            beside = os.path.join(os.path.dirname(os.path.abspath(path)), parent)
            parent = beside if os.path.exists(beside) else parent
        path = parent
    if default_path is not None:
        with open(default_path, 'r') as f:
            chain.append(yaml.safe_load(f) or {})
    cfg = {}
    for special in reversed(chain):
        update_recursive(cfg, special)
    return cfg
