"""Linear / Conv{1,2,3}d LocalReparameterization: the local reparameterization trick (Kingma, Salimans & Welling 2015; the naming
follows TensorFlow Probability's DenseLocalReparameterization).  Not in the reference.

The layers sample the pre-activations instead of the weights (BTX-LRT v1):

    m = x (*) mu_W + mu_b ,  v = x^2 (*) sigma_W^2 + sigma_b^2 ,  out = m + sqrt(v) * zeta ,  zeta ~ N(0, 1) per OUTPUT element

Constructor arguments, parameter / buffer names, state_dict() keys, kl_loss(), return_kl and dnn_to_bnn_flag are those of the
`...Reparameterization` classes: a Reparameterization checkpoint loads into these layers and back, and the KL is the same function
of (mu, rho).  For a Linear layer the marginal of every output element is exactly Reparameterization's; a convolution draws its
own zeta at every output position, which matches the marginal of each output element of a shared-weight sample but not the joint
over positions.  There is no INT8 twin: prepare() raises.
"""
from ..base_variational_layer import _VariationalNd
from ..._lib import BtxError

__all__ = ['LinearLocalReparameterization', 'Conv1dLocalReparameterization', 'Conv2dLocalReparameterization',
           'Conv3dLocalReparameterization']


class _LocalReparameterizationNd(_VariationalNd):
    _family = "lrt"

    def prepare(self):
        raise BtxError("%s has no quantized form: prepare() / bnn_to_qbnn cover the Reparameterization and Flipout layers only"
                       % type(self).__name__)


class LinearLocalReparameterization(_LocalReparameterizationNd):
    """Linear with the local reparameterization trick; the surface of LinearReparameterization."""
    _nd, _transposed = 0, False

    def __init__(self, in_features, out_features, prior_mean=0, prior_variance=1, posterior_mu_init=0,
                 posterior_rho_init=-3.0, bias=True):
        super().__init__()
        self.posterior_mu_init = posterior_mu_init,
        self.posterior_rho_init = posterior_rho_init,
        self._setup(in_features, out_features, 1, 1, 0, 1, 1, 0, prior_mean, prior_variance,
                    posterior_mu_init, posterior_rho_init, bias, check_groups=False)


class Conv1dLocalReparameterization(_LocalReparameterizationNd):
    """Conv1d with the local reparameterization trick; the surface of Conv1dReparameterization."""
    _nd, _transposed = 1, False

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, prior_mean=0, prior_variance=1, posterior_mu_init=0, posterior_rho_init=-3.0, bias=True):
        super().__init__()
        self.posterior_mu_init = posterior_mu_init,
        self.posterior_rho_init = posterior_rho_init,
        self._setup(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, 0,
                    prior_mean, prior_variance, posterior_mu_init, posterior_rho_init, bias,
                    check_groups=True)


class Conv2dLocalReparameterization(_LocalReparameterizationNd):
    """Conv2d with the local reparameterization trick; the surface of Conv2dReparameterization."""
    _nd, _transposed = 2, False

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, prior_mean=0, prior_variance=1, posterior_mu_init=0, posterior_rho_init=-3.0, bias=True):
        super().__init__()
        self.posterior_mu_init = posterior_mu_init,
        self.posterior_rho_init = posterior_rho_init,
        self._setup(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, 0,
                    prior_mean, prior_variance, posterior_mu_init, posterior_rho_init, bias,
                    check_groups=True)


class Conv3dLocalReparameterization(_LocalReparameterizationNd):
    """Conv3d with the local reparameterization trick; the surface of Conv3dReparameterization (positional prior / posterior
    arguments, as there)."""
    _nd, _transposed = 3, False

    def __init__(self, in_channels, out_channels, kernel_size, prior_mean, prior_variance, posterior_mu_init, posterior_rho_init, stride=1, padding=0, dilation=1, groups=1, bias=True):
        super().__init__()
        self.posterior_mu_init = posterior_mu_init,
        self.posterior_rho_init = posterior_rho_init,
        self._setup(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, 0,
                    prior_mean, prior_variance, posterior_mu_init, posterior_rho_init, bias,
                    check_groups=True)
