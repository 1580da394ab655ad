from videoswap_amd.dift import DIFTDemo as DIFT_Demo, SDFeaturizer  # noqa: F401
