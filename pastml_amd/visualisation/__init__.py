"""What this project has of PastML's visualisation layer: the vertical and horizontal steps of the tree compressor and their Pajek network."""
