from peekvit_amd import losses as _impl

globals().update({k: v for k, v in vars(_impl).items() if not k.startswith("__")})
