"""models_baseline: the posenets the augmentation trains."""
