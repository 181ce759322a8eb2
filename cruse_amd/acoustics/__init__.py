from .df_features import DfFeatures, ExponentialUnitNorm, get_norm_alpha  # noqa: F401
