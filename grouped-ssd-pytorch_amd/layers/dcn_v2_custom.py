"""DCN / DCNv2 / dcn_v2_conv (drop-in names for ssd_liverdet/layers/dcn_v2_custom.py): the modules of gssd.modules and the
HIP autograd op of gssd.dcn_op (``_DCNv2.apply`` takes the reference's argument order)."""
from gssd.dcn_op import _DCNv2, dcn_v2_conv
from gssd.modules import DCN, DCNv2

__all__ = ['DCN', 'DCNv2', 'dcn_v2_conv', '_DCNv2']
