"""--optimizer choices and the default hyper-parameters of those that have their own
(tf_cnn_benchmarks --rmsprop_* / --adam_* defaults). Plain data, no imports: the flag table
(bench/flags.py) and the Trainer both read it."""

OPT_DEFAULTS = {
    "sgd": {},
    "momentum": {},  # --momentum, the Trainer's own argument
    "rmsprop": {"decay": 0.9, "momentum": 0.9, "epsilon": 1.0},
    "adam": {"beta1": 0.9, "beta2": 0.999, "epsilon": 1e-8},
}
