"""``ldpc_amd.bpgd_decoder`` -- BP with guided decimation on MI355X (no counterpart in the reference): rounds of min-sum iterations with the
most reliable bit frozen after every unsolved round, decoded in one call (``ldpc_hip_bp_set_decimation``)."""
from ldpc_amd.bpgd_decoder._bpgd_decoder import BpgdDecoder, decimation_schedule, lane_edge_route, lane_node_takes

__all__ = ["BpgdDecoder", "decimation_schedule", "lane_edge_route", "lane_node_takes"]
