# SVAO with the RASTER stochastic depth map (SVAO's StochasticDepthImpl::Raster, selected here by the
# `stochImpl` property): GBufferRaster -> LinearizeDepth / CompressNormals -> SVAO, whose nested graph
# holds the StochasticDepthMap pass fed by SVAO.gbufferDepth; and a standalone StochasticDepthMap pass on
# the same G-buffer depth.  No culling, exact numerics.  Loaded by tests/test_sd_raster.py (planned) and
# tests/test_gpu_graph_sd_raster.py (executed) with rsd.graph.load_script.
from falcor import *

def render_graph_svao_raster_sd():
    g = RenderGraph('SVAORasterSD')
    g.create_pass('GBufferRaster', 'GBufferRaster', {'outputSize': 'Default', 'samplePattern': 'Center', 'forceCullMode': True, 'cull': 'None'})
    g.create_pass('LinearizeDepth', 'LinearizeDepth', {'depthFormat': 'R32Float'})
    g.create_pass('CompressNormals', 'CompressNormals', {'viewSpace': True, 'use16Bit': True})
    g.create_pass('SVAO', 'SVAO', {'radius': 6.0, 'primaryDepthMode': 'SingleDepth', 'secondaryDepthMode': 'StochasticDepth', 'exponent': 2.0, 'thickness': 0.0, 'stochMapDivisor': 1, 'dualAO': False, 'alphaTest': True, 'stochGuardBand': 16, 'stochSamples': 4, 'cullMode': 'None', 'numerics': 'Exact', 'stochImpl': 'Raster'})
    g.create_pass('SDMap', 'StochasticDepthMap', {'SampleCount': 8, 'Alpha': 0.2, 'CullMode': 'None', 'linearize': True, 'depthFormat': 'D32Float', 'AlphaTest': True, 'Implementation': 'Default', 'RayInterval': True})
    g.add_edge('GBufferRaster.depth', 'LinearizeDepth.depth')
    g.add_edge('GBufferRaster.depth', 'SVAO.gbufferDepth')
    g.add_edge('GBufferRaster.depth', 'SDMap.depthMap')
    g.add_edge('GBufferRaster.faceNormalW', 'CompressNormals.normalW')
    g.add_edge('LinearizeDepth.linearDepth', 'SVAO.depth')
    g.add_edge('CompressNormals.normalOut', 'SVAO.normals')
    g.mark_output('SVAO.ao')
    g.mark_output('SDMap.stochasticDepth')
    return g

SVAORasterSD = render_graph_svao_raster_sd()
try: m.addGraph(SVAORasterSD)
except NameError: None
