"""What this project has of PastML's visualisation layer: the vertical step of the tree compressor and its Pajek network."""
