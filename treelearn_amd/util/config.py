"""Config files: the reference's `get_config` (tree_learn/util/parser.py:23-60) without `munch`.

A main YAML may name other YAML files under `default_args`; each is loaded, the main file's values for keys both define are written
into it (nested dicts key by key, anything else replaced), and the result is merged over the main file.  The returned object is a
dict whose keys are also attributes, nested dicts included.

The reference opens `default_args` paths relative to the working directory (its commands are run from the repository root).  Here a
path is tried as given first; if no such file exists it is tried relative to each ancestor directory of the main config file, nearest
first, so `python -m treelearn_amd.util.trainer --config /some/where/configs/training/train.yaml` works from any directory.
"""
import os.path as osp

import yaml


class Config(dict):
    """dict with attribute access; `Config.from_dict` converts nested dicts (also inside lists and tuples)."""

    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError:
            raise AttributeError(key) from None

    def __setattr__(self, key, value):
        self[key] = value

    def __delattr__(self, key):
        try:
            del self[key]
        except KeyError:
            raise AttributeError(key) from None

    @classmethod
    def from_dict(cls, obj):
        if isinstance(obj, dict):
            return cls((k, cls.from_dict(v)) for k, v in obj.items())
        if isinstance(obj, (list, tuple)):
            return type(obj)(cls.from_dict(v) for v in obj)
        return obj

    def to_dict(self):
        return to_dict(self)


def to_dict(obj):
    """Plain dicts again (parser.py:62-70), e.g. for `TreeLearn(**config.model)` or yaml.dump."""
    if isinstance(obj, dict):
        return {k: to_dict(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(to_dict(v) for v in obj)
    return obj


def load_yaml_file(filepath):
    with open(filepath, 'r') as file:
        return yaml.safe_load(file)


def _override(default, main):
    """Write the main file's values into a default section: dict into dict key by key, anything else replaces (parser.py:55-60)."""
    for key, value in main.items():
        if isinstance(value, dict) and isinstance(default.get(key), dict):
            _override(default[key], value)
        else:
            default[key] = value


def resolve(path, config_path):
    """`path` as given if it exists, else relative to the ancestors of config_path's directory, nearest first."""
    if osp.exists(path) or osp.isabs(path):
        return path
    d = osp.dirname(osp.abspath(config_path))
    while True:
        cand = osp.join(d, path)
        if osp.exists(cand):
            return cand
        parent = osp.dirname(d)
        if parent == d:
            return path                                    # open() then reports the path as written
        d = parent


def get_config(config_path):
    main_cfg = load_yaml_file(config_path)
    default_args = main_cfg.pop('default_args', None)
    if default_args is not None:
        for path in default_args:
            default_config = load_yaml_file(resolve(path, config_path))
            _override(default_config, {k: v for k, v in main_cfg.items() if k in default_config})
            main_cfg.update(default_config)
    return Config.from_dict(main_cfg)
