from ldpc_amd.monte_carlo_simulation.mcs import MonteCarloBscSimulation
from ldpc_amd.monte_carlo_simulation.dem_mcs import MonteCarloDemSimulation

__all__ = ["MonteCarloBscSimulation", "MonteCarloDemSimulation"]
