"""makani_amd — MI355X-native SFNO / spherical-harmonic-transform hot path behind
makani's nn.Module plug-in API.  HIP kernels live in ``csrc/`` behind the C ABI of
``include/makani_amd.h``; this package is the host-side mirror of the reference interface."""
from .sht import RealSHT, InverseRealSHT, RealVectorSHT, InverseRealVectorSHT
from .distributed import DistributedRealVectorSHT, DistributedInverseRealVectorSHT
from .spectral_conv import SpectralConv
from .layers import MLP, EncoderDecoder, InstanceNorm2d, PointwiseConv, GeometricInstanceNormS2
from .sfno import SphericalFourierNeuralOperatorNet, NeuralOperatorBlock, SpectralFilterLayer
from .losses import CRPSLoss, GradientCRPSLoss, VortDivCRPSLoss, GeometricLpLoss, GridQuadrature, SpectralCRPSLoss, SpectralLpLoss, SpectralH1Loss
from .losses import LpEnergyScoreLoss, L2EnergyScoreLoss, SobolevEnergyScoreLoss, SpectralL2EnergyScoreLoss
from .losses import SpectralAMSELoss, EnsembleNLLLoss, GaussianMMDLoss
from .losses import SpectralCoherenceLoss, CoherenceRegularization, SpectralRegularization, EnsembleGramFn
from .losses import HydrostaticBalanceLoss, DriftRegularization, LossHandler
from .metrics import (GeometricL1, GeometricRMSE, GeometricACC, GeometricSpread, GeometricSSR, GeometricCRPS, GeometricRankHistogram,
                      deterministic_sums)
from .metric import MetricsHandler, MetricRollout, Quadrature, SimpsonQuadrature, TrapezoidQuadrature
from .stepper import MultiStepWrapper, SingleStepWrapper
from .disco import DiscreteContinuousConvS2, ResampleS2
from .fcn3 import AtmoSphericNeuralOperatorNet
from .preprocessor import Preprocessor2D
from .noise import BaseNoiseS2, IsotropicGaussianRandomFieldS2, DiffusionNoiseS2, DummyNoiseS2, InputNoise, build_noise, noise_seed_reflect
from .rollout_buffer import MeanStdBuffer, TemporalAverageBuffer, SpectrumAverageBuffer, ZonalSpectrumAverageBuffer, power_spectrum
from .constraints import (ConstraintsWrapper, HydrostaticBalanceProjection, NonNegativeConstraint, constrain_model_handle,
                          get_matching_channels_pl)
from .interpolant import InterpolationWrapper, TimeAwareInterpolationWrapper, StochasticInterpolantWrapper
from .imputation import MLPImputation, ConstantImputation
from .fcn31 import AtmoSphericNeuralOperatorNet31, LearnablePositionEmbedding

__all__ = ["RealSHT", "InverseRealSHT", "RealVectorSHT", "InverseRealVectorSHT",
           "DistributedRealVectorSHT", "DistributedInverseRealVectorSHT", "GradientCRPSLoss", "VortDivCRPSLoss", "SpectralConv", "MLP", "EncoderDecoder", "InstanceNorm2d", "PointwiseConv",
           "SphericalFourierNeuralOperatorNet", "NeuralOperatorBlock", "SpectralFilterLayer", "GeometricLpLoss",
           "GridQuadrature", "SpectralLpLoss", "SpectralH1Loss", "CRPSLoss", "SpectralCRPSLoss", "GeometricInstanceNormS2", "MultiStepWrapper", "SingleStepWrapper",
           "DiscreteContinuousConvS2", "ResampleS2", "AtmoSphericNeuralOperatorNet",
           "LpEnergyScoreLoss", "L2EnergyScoreLoss", "SobolevEnergyScoreLoss", "SpectralL2EnergyScoreLoss",
           "SpectralAMSELoss", "EnsembleNLLLoss", "GaussianMMDLoss",
           "SpectralCoherenceLoss", "CoherenceRegularization", "SpectralRegularization", "EnsembleGramFn",
           "HydrostaticBalanceLoss", "DriftRegularization", "LossHandler",
           "GeometricL1", "GeometricRMSE", "GeometricACC", "GeometricSpread", "GeometricSSR", "GeometricCRPS", "GeometricRankHistogram",
           "deterministic_sums", "MetricsHandler", "MetricRollout", "Quadrature", "SimpsonQuadrature", "TrapezoidQuadrature",
           "BaseNoiseS2", "IsotropicGaussianRandomFieldS2", "DiffusionNoiseS2", "DummyNoiseS2", "InputNoise", "build_noise",
           "noise_seed_reflect", "Preprocessor2D",
           "MeanStdBuffer", "TemporalAverageBuffer", "SpectrumAverageBuffer", "ZonalSpectrumAverageBuffer", "power_spectrum",
           "ConstraintsWrapper", "HydrostaticBalanceProjection", "NonNegativeConstraint", "constrain_model_handle",
           "get_matching_channels_pl",
           "InterpolationWrapper", "TimeAwareInterpolationWrapper", "StochasticInterpolantWrapper",
           "MLPImputation", "ConstantImputation", "AtmoSphericNeuralOperatorNet31", "LearnablePositionEmbedding"]
